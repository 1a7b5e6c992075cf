"""`python -m gulon_amd`: the reference's query commands (command/Main.scala:8-11).

  query-words -i INDEX [-k N] [FILE]   command/QueryWords.scala: one word per line of FILE (or stdin), printed as
                                       `word: w1,w2,...` or `word: not found`, in input order
  query -i INDEX [-k N] FILE           command/Query.scala: a word2vec text file of query vectors, printed as
                                       `key: w1,w2,...`

Input is UTF-8; lines end as java.io.BufferedReader.readLine ends them (\\n, \\r or \\r\\n).  Words are queried in
batches; the output is the same as querying them one at a time."""
import argparse
import re
import sys

_EOL = re.compile(r"\r\n|\r|\n")
CHUNK = 1024        # lines per batch of query-words


def read_lines(data: bytes):
    """BufferedReader.readLine over the UTF-8 text in `data` (malformed input replaced, as InputStreamReader does)."""
    text = data.decode("utf-8", "replace")
    if text == "":
        return []
    lines = _EOL.split(text)
    if text[-1] in "\r\n":          # a final terminator ends the last line and starts none
        lines.pop()
    return lines


def _positive(s):
    try:
        v = int(s)
    except ValueError:
        raise argparse.ArgumentTypeError(f"invalid integer: {s!r}")
    if v <= 0:
        raise argparse.ArgumentTypeError("must be at least 1")
    return v


def _parser():
    p = argparse.ArgumentParser(prog="python -m gulon_amd", description="query a Gulon nearest neighbour index")
    sub = p.add_subparsers(dest="command", required=True)
    for name, help_, need_file in (("query-words", "query nearest neighbour index by word", False),
                                   ("query", "query nearest neighbour index", True)):
        s = sub.add_parser(name, help=help_, description=help_)
        s.add_argument("-k", "--neighbours", type=_positive, default=1, metavar="num",
                       help="number of nearest neighbours to return")
        s.add_argument("-i", "--index", required=True, metavar="file", help="path to ANN index")
        s.add_argument("file", nargs=None if need_file else "?", metavar="file")
    return p


def _line(word, result):
    return f"{word}: not found" if result is None else f"{word}: {','.join(result.words)}"


def query_words(index, k, lines, write):
    for s in range(0, len(lines), CHUNK):
        part = lines[s:s + CHUNK]
        for word, result in zip(part, index.batch_query_by_words(k, part)):
            write(_line(word, result) + "\n")


def query(index, k, vectors, write):
    results = index.batch_query(k, vectors.data) if vectors.size else []
    for word, result in zip(vectors.words, results):
        write(_line(word, result) + "\n")


def main(argv=None, stdin=None, stdout=None, load=None):
    """Returns the exit code.  stdin / stdout: binary streams (default: the process's); load: path -> index with
    batch_query_by_words / batch_query (default WordIndex.load)."""
    args = _parser().parse_args(argv)
    stdin = stdin if stdin is not None else sys.stdin.buffer
    stdout = stdout if stdout is not None else sys.stdout.buffer
    if load is None:
        from .word_index import WordIndex
        load = WordIndex.load

    def write(text):
        stdout.write(text.encode("utf-8"))

    if args.command == "query-words":
        index = load(args.index)
        if args.file is None:
            data = stdin.read()
        else:
            with open(args.file, "rb") as fh:
                data = fh.read()
        query_words(index, args.neighbours, read_lines(data), write)
    else:
        from .word_vectors import read_word2vec
        vectors = read_word2vec(args.file)
        index = load(args.index)
        query(index, args.neighbours, vectors, write)
    stdout.flush()
    return 0
