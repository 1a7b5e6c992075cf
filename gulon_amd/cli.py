"""`python -m gulon_amd`: the reference's four commands (command/Main.scala:7-11), `inspect`, `update`, `build-fine`,
`analogies`, `similarity`, `translate` and `align`.

  build-index -d l2|cosine -o INDEX [-k N] [-m N] [-n N] [-p [--partitions N] [-l N]] [-R ROTATION [--rotation-rounds N]]
              FILE
                                       command/BuildIndex.scala: a word2vec text file -> an index file; the text is
                                       parsed on the device (word_vectors.read_word2vec_device) and every later stage
                                       runs there too (build.build_index)

  query-words -i INDEX [-k N] [-x [--method add|mul]] [-v VECTORS [--exact] | -f FINE] [-c N] [FILE]
                                       command/QueryWords.scala: one word per line of FILE (or stdin), printed as
                                       `word: w1,w2,...` or `word: not found`, in input order
  query -i INDEX [-k N] [-v VECTORS [--exact] | -f FINE] [-c N] FILE
                                       command/Query.scala: a word2vec text file of query vectors, printed as
                                       `key: w1,w2,...`
  test -v VECTORS -i INDEX [-s SIZE] [-e ERROR] [[-f FINE] -c N]
                                       command/Test.scala: the recall of an index file against the exact neighbours in
                                       the word2vec text file it was built from, `R@k: mean +/- stdDev` for
                                       k = 1 ... 1000 over SIZE sampled vectors (tests_recall.Tests; the vectors are
                                       read, the exact neighbours found and the results evaluated on the device)

  inspect -i INDEX [-v VECTORS [-w N]]
                                       (not in the reference) the diagnostics of an index file (inspect.IndexReport): its
                                       shape and, per quantizer, how many centroids are used, the largest share of one
                                       centroid and the entropy of the codes; with -v -- the word2vec text file it was
                                       built from -- also the mean and relative squared error of its rows against their
                                       original vectors, the mean error per quantizer and the N (default 10) words with
                                       the largest error.  Counted and summed on the device (csrc/inspect.hip)

  update -i INDEX -o OUTPUT [-a VECTORS] [-x WORDS]
                                       (not in the reference) add, replace and remove words of an index file without
                                       retraining (update.py, csrc/update.hip): the words of WORDS (one per line) are
                                       removed first, then every word of the word2vec text file VECTORS is added, or
                                       replaced if the index still has it -- encoded by the index's own code books on the
                                       device, read normalised for a cosine index.  Kept words keep their codes.  Not for
                                       a partitioned (grouped) index

  build-fine -i INDEX -v VECTORS -o OUTPUT [-k N] [-m N] [-n N]
                                       (not in the reference) the fine index of an index file (fine.py, csrc/fine.hip): a
                                       second quantizer over the residuals the index leaves against the word2vec text
                                       file VECTORS it was built from (read normalised for a cosine index), written as an
                                       ordinary sorted l2 index file.  -k / -m / -n as for build-index

  analogies -i INDEX [-k 1,5,10] [--lowercase] [--method add|mul] [-v VECTORS [--exact | -c N]] FILE
                                       (not in the reference) the analogy accuracy of an index file (analogies.py,
                                       csrc/analogy.hip) on FILE, questions in the questions-words.txt format: `: name`
                                       opens a section, every other line is `a b c d`.  A question is right at k when d
                                       is among the first k neighbours of b - a + c that are none of a, b, c.  One line
                                       per section, `name: @1 0.7312 @5 0.8103 @10 0.8521 (n = 506, skipped 12)` -- n
                                       the questions asked, skipped those with a word the index lacks -- and a `total:`
                                       line.  The target is the index alone; with -v its form refined against that
                                       word2vec text file (-c N candidates, default 10 * the largest k); with -v --exact
                                       the true vectors of the index's words (WordIndex.exact).  Composed, queried and
                                       scored on the device.  -f, -r and -R are not offered: a rotated index needs no
                                       rotation file when it is evaluated alone or with --exact (the stored rows are
                                       composed where they live, and --exact reads the index for its words only);
                                       -v -c on a rotated index is outside this command.  --method mul ranks the
                                       rows by 3CosMul instead (csrc/cosmul.hip): s(d, b) * s(d, c) / (s(d, a) + 0.001)
                                       with s = (1 + cos) / 2, for a flat cosine index alone or with -v --exact.
                                       query-words -x --method mul answers expressions the same way

  similarity -i INDEX [--lowercase] [-v VECTORS --exact] FILE
                                       (not in the reference) Spearman's rank correlation between the human scores of a
                                       word-pair similarity file (WordSim-353, SimLex-999, MEN, RW ...) and the distances
                                       the index puts between the words of every pair (similarity.py, csrc/pairs.hip).
                                       FILE: lines of `word1 word2 score`; blank lines and lines starting with # are
                                       skipped; `: name` opens a section, so several benchmarks fit in one file.  One line
                                       per section, `name: rho 0.6532 (n = 353, skipped 12, dropped 0)` -- n the pairs
                                       ranked, skipped those with a word the index lacks, dropped those whose distance is
                                       NaN -- and a `total:` line over the pooled pairs.  rho is that of the scores
                                       against the similarity, i.e. the negated rho of the distances.  The target is the
                                       index alone; with -v --exact the true vectors of the index's words.  Distances
                                       and ranks are computed on the device.  -R is not offered: distances between stored
                                       rows need no rotation

  translate -i TARGET -s SOURCE [--method nn|csls|isf] [-n 10] [--beta 30] [--isf-sources N] [-k 10]
            [-v VECTORS --exact] [-R ROTATION] [-a MAP] [--lowercase] (WORDS | -e DICTIONARY [--ranks])
                                       (not in the reference) word translation between two aligned embedding spaces
                                       (csls.py, csrc/offset.hip).  TARGET is an index file over the target language's
                                       vectors, SOURCE a word2vec text file of the source language's, already mapped
                                       into the target's space (read normalised for a cosine index).  Every line of
                                       WORDS is a source word, printed as `word: t1,t2,...` with its -k (default 10)
                                       nearest target words, or `word: not found`.  --method nn ranks by the index's
                                       distance; csls (a cosine index, flat or built with -p, or -v --exact; a -p index
                                       answers from the groups its strategy searches) by CSLS: the distance plus the
                                       mean similarity of the target word to its -n (default 10) nearest source words,
                                       which demotes the hubs that are near everything.  isf (the same indexes) ranks
                                       by the inverted softmax of Smith et al. 2017 (softmax.py, csrc/logsumexp.hip):
                                       the distance plus (2 / beta) * log sum exp(-(beta / 2) * distance) over ALL the
                                       source words, --beta (default 30) the inverse temperature, --isf-sources N the
                                       sum over the N most frequent source words only (the first N lines of SOURCE); its lines are those of csls with `isf`
                                       as the method name.  --beta and --isf-sources without --method isf are usage
                                       errors.  -e DICTIONARY replaces WORDS:
                                       lines of `source target` (MUSE's format, a source word may have several lines),
                                       and one line is printed, `csls: @1 0.6120 @5 0.8010 @10 0.8522 (n = 1500,
                                       skipped 12)` -- the precision at -k 1,5,10, n the source words asked, skipped the
                                       pairs with a word either side lacks.  --ranks (with -e) adds a second line,
                                       `csls ranks: mrr 0.7012 median 1 mean 37.42 @1 0.6120 @5 0.8010 @100 0.9312
                                       (n = 1500, unranked 3, skipped 12)`: the rank of a word is the number of target
                                       words ahead of its best gold translation, counted on the device over ALL the
                                       target's words (ranks.py, csrc/rank.hip) -- mrr the mean of 1 / (rank + 1),
                                       median and mean over the ranked words (1-based), unranked the words none of
                                       whose translations can be ranked.  The depths of -k may then exceed 63.  With
                                       --method nn equal distances are ordered by row, which is not the tie order of
                                       the query behind the first line.  Not on a -p index (`error: ...`, status 1).
                                       -v VECTORS --exact: the target is the true
                                       vectors of the index's words.  -R ROTATION: the index was built with build-index
                                       -R, and the source vectors are rotated after they are read (not with --exact).
                                       -a MAP: SOURCE is NOT mapped yet; the map `align` wrote is applied to its vectors
                                       on the device after they are read, before -R's rotation

  align -s SOURCE -t TARGET (-d DICTIONARY | --identical) -o MAP [--rounds 5] [--max-rank 15000] [-n 10] [--lowercase]
                                       (not in the reference) learn the orthogonal map that takes the vectors of SOURCE
                                       into the space of TARGET (alignment.py, csrc/alignment.hip): MUSE's supervised
                                       recipe.  Both are word2vec text files in frequency order, read normalised and NOT
                                       sorted.  The seed is DICTIONARY, lines of `source target`, or with --identical the
                                       words spelt the same on both sides; an orthogonal Procrustes solve on it, then
                                       --rounds refinements, each solving again on the pairs among the first --max-rank
                                       words of either side that are each other's CSLS best match (-n neighbours behind
                                       the mean similarities).  Printed: `seed: 4821 pairs, skipped 179`, per round
                                       `round 2: mutual 9312 of 15000, criterion 0.612345` -- the criterion the mean
                                       cosine of the 10 000 most frequent source words with their best match -- and
                                       `chosen: round 3`, the round whose map is written to MAP (a rotation file, as
                                       build-index -R writes them) for translate -a

-f FINE on the query commands and on test (not in the reference): as -v / -c, but the candidates are re-ranked by their
distance to the index's row plus the fine index's row of the same word (fine.FineRefinedIndex) -- no original vectors in
memory.  FINE is a file written by build-fine.  Not together with -v (on the query commands) or -r; works with -x.  On
test, -f needs -c, and the R@k lines are prefixes of one result per query exactly as described for -c below.

-v VECTORS on the query commands (not in the reference): the index's N candidates per query (-c, default 10 * k) are
re-ranked by their exact distance to the original vectors of that word2vec text file, and the k nearest are printed
(refine.RefinedIndex).  test -c N reports the recall of that refined index.  The recall harness asks ONE query per
sampled vector at the largest k it kept and scores prefixes of the answer, so every R@k line is a prefix of one refined
result -- the max(N, largest k) candidates re-ranked, the largest k kept -- not a refined query at that k.

--exact on the query commands (not in the reference; exact.py, csrc/exact.hip): with -v VECTORS, the TRUE neighbours among
the original vectors instead of re-ranked candidates -- brute force over every word of the index on the device
(WordIndex.exact).  The index file supplies the words, the metric and the row order; query-words asks with the word's
original vector, so the word itself comes first.  The output lines are those of the plain command.  Not together with
-c, -f, -r, -x or -R.

-x/--expressions on query-words (not in the reference): every line is an expression `word (op word)*`, split on
whitespace, op one of the stand-alone tokens + and - (weights +1 and -1; a word may itself contain + or -, which is why
this is opt-in).  The query is the sum of the index's vectors of the words with those weights (expressions.py), composed
on the device; the words of the line are left out of its answer, so a line of one word prints that word's neighbours
without the word itself.  A line is printed as `line: w1,w2,...`, `line: not found` if any of its words is absent, or
`line: invalid expression` (an empty line, a leading or trailing operator, two operators or two words in a row).
Works together with -v / -c.

-R/--rotation FILE (not in the reference; rotation.py, csrc/rotate.hip): an orthogonal rotation learned before quantizing.
build-index -R FILE [--rotation-rounds N] learns it on the vectors as read (N refinement rounds, default 4; with -p too it
is learned for the flat quantizer), writes it to FILE, rotates the vectors on the device and builds the index over them.
The query commands take the same -R FILE: the loaded index is wrapped (rotation.RotatedWordIndex) before -v, -f, -r and -x
apply, so query vectors are rotated on their way in and -v's vectors once on the device.  On test, inspect, build-fine and
update, -R FILE rotates the vectors file (-a for update) after reading it; the index file is used as it is.

Input is UTF-8; lines end as java.io.BufferedReader.readLine ends them (\\n, \\r or \\r\\n).  Words are queried in
batches; the output is the same as querying them one at a time."""
import argparse
import math
import re
import sys
from dataclasses import dataclass
from typing import Optional

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


def _positive_float(s):
    try:
        v = float(s)
    except ValueError:
        raise argparse.ArgumentTypeError(f"invalid number: {s!r}")
    if not (math.isfinite(v) and v > 0):
        raise argparse.ArgumentTypeError("must be a finite number above 0")
    return v


@dataclass(frozen=True)
class BuildConfig:
    """BuildIndex.Config (BuildIndex.scala:15-22); partitioned: build.Partitioned or None."""
    metric: str
    num_clusters: int
    num_quantizers: int
    max_iterations: int
    partitioned: Optional[object]
    output: str
    input: str
    rotation: Optional[str] = None        # -R: learn a rotation first and write it to this file
    rotation_rounds: int = 4              # --rotation-rounds: refinement rounds after the initial rotation


def _integer(s):
    try:
        return int(s)
    except ValueError:
        raise argparse.ArgumentTypeError(f"invalid integer: {s!r}")


def _clusters(s):                                            # BuildIndex.scala:29-34
    v = _integer(s)
    if v <= 0:
        raise argparse.ArgumentTypeError("clusters must be at least 1")
    if v > 65536:
        raise argparse.ArgumentTypeError("too many clusters, must be at most 65536")
    return v


def _metric(s):                                              # BuildIndex.scala:35-41
    if s not in ("l2", "cosine"):
        raise argparse.ArgumentTypeError(f"unsupported metric: {s}")
    return s


@dataclass(frozen=True)
class RecallConfig:
    """Test.Options (Test.scala:11-15); epsilon is a binary32."""
    vectors: str
    index: str
    sample_size: int
    epsilon: float
    candidates: Optional[int] = None      # -c: the recall of the index refined over this many candidates
    fine: Optional[str] = None            # -f: refined against this fine index file instead of the vectors
    rotation: Optional[str] = None        # -R: the index was built over vectors rotated by this file


@dataclass(frozen=True)
class FineConfig:
    """build-fine: the index file, the word2vec text it was built from, the output, and build-index's quantizer options."""
    index: str
    vectors: str
    output: str
    num_clusters: int = 256
    num_quantizers: int = 25
    max_iterations: int = 100
    rotation: Optional[str] = None        # -R: the index was built over vectors rotated by this file


@dataclass(frozen=True)
class InspectConfig:
    index: str
    vectors: Optional[str] = None         # -v: compare the index with the vectors it was built from
    worst: int = 10                       # -w: words with the largest error to list
    rotation: Optional[str] = None        # -R: the index was built over vectors rotated by this file


@dataclass(frozen=True)
class UpdateConfig:
    index: str
    output: str
    add: Optional[str] = None             # -a: word2vec text of the words to add or replace
    remove: Optional[str] = None          # -x: one word per line to remove
    rotation: Optional[str] = None        # -R: the index was built over vectors rotated by this file


@dataclass(frozen=True)
class AnalogiesConfig:
    index: str
    questions: str
    ks: tuple = (1, 5, 10)                # -k: the depths reported, ascending
    lowercase: bool = False               # --lowercase: lower the questions' words
    vectors: Optional[str] = None         # -v: refine against (or, exact, ask) the vectors the index was built from
    exact: bool = False                   # --exact: the true vectors of the index's words are the target
    candidates: Optional[int] = None      # -c: candidates of the refined form (default 10 * the largest k)
    method: str = "add"                   # --method: add (3CosAdd, the neighbours of b - a + c) or mul (3CosMul)


@dataclass(frozen=True)
class SimilarityConfig:
    index: str
    pairs: str
    lowercase: bool = False               # --lowercase: lower the pairs' words
    vectors: Optional[str] = None         # -v: the vectors the index was built from (with --exact)
    exact: bool = False                   # --exact: the true vectors of the index's words are the target


@dataclass(frozen=True)
class TranslateConfig:
    index: str
    source: str                           # -s: word2vec text of the source language, aligned with the target
    words: Optional[str] = None           # the file of source words to translate ...
    dictionary: Optional[str] = None      # ... or -e: the dictionary to evaluate
    method: str = "nn"                    # --method: nn (the index's distance) or csls
    neighbours: int = 10                  # -n: the K of CSLS's mean similarities
    k: int = 10                           # -k: translations printed per word
    ks: tuple = (1, 5, 10)                # -k with -e: the depths reported, ascending
    lowercase: bool = False               # --lowercase: lower the words of WORDS / the dictionary
    vectors: Optional[str] = None         # -v: the vectors the index was built from (with --exact)
    exact: bool = False                   # --exact: the true vectors of the index's words are the target
    rotation: Optional[str] = None        # -R: the index was built over vectors rotated by this file
    alignment: Optional[str] = None       # -a: the map of the source vectors into the target's space (align)
    ranks: bool = False                   # --ranks with -e: the line of rank statistics after the precision line
    # (`ranks` stays the last field: the options of --method isf are IsfTranslateConfig's, these are what nn and csls see)
    beta = 30.0
    isf_sources = None


@dataclass(frozen=True)
class IsfTranslateConfig(TranslateConfig):
    """TranslateConfig of --method isf: the same fields, then the inverted softmax's own."""
    beta: float = 30.0                    # --beta: the inverse temperature of the inverted softmax
    isf_sources: Optional[int] = None     # --isf-sources: normalise over the first N words of the FILE (None: all)


@dataclass(frozen=True)
class AlignConfig:
    source: str                           # -s: word2vec text of the source language, in frequency order
    target: str                           # -t: the same of the target language
    output: str                           # -o: the map, a rotation file
    dictionary: Optional[str] = None      # -d: the seed dictionary ...
    identical: bool = False               # ... or --identical: the words spelt the same on both sides
    rounds: int = 5                       # --rounds: refinement rounds after the seed
    max_rank: int = 15000                 # --max-rank: the most frequent words of either side that take part
    neighbours: int = 10                  # -n: the K of CSLS's mean similarities
    lowercase: bool = False               # --lowercase: lower the dictionary's words


def _depths(s):
    try:
        ks = tuple(int(t) for t in s.split(","))
    except ValueError:
        raise argparse.ArgumentTypeError(f"invalid list of integers: {s!r}")
    if not ks or len(ks) > 16 or ks[0] < 1 or any(b <= a for a, b in zip(ks, ks[1:])):
        raise argparse.ArgumentTypeError("must be 1 to 16 ascending integers from 1 up, separated by commas")
    return ks


def _sample_size(s):                                     # Test.scala:24-28
    if _integer(s) <= 0:
        raise argparse.ArgumentTypeError("must be greater than 0")
    return _integer(s)


def _epsilon(s):                                             # Test.scala:29-33
    from .word_vectors import parse_float
    try:
        v = parse_float(s)
    except ValueError:
        raise argparse.ArgumentTypeError(f"invalid float: {s!r}")
    if not v >= 0:
        raise argparse.ArgumentTypeError("must be non-negative")
    return v


def _rounds(s):
    v = _integer(s)
    if v < 0:
        raise argparse.ArgumentTypeError("must not be negative")
    return v


_ROTATED_VECTORS = ("rotation file the index was built with (build-index -R): the vectors are rotated on the device after "
                    "they are read")


def _rotated(path, vectors):
    """The word vectors as read, or with -R rotated on the device by that file (the unrotated matrix is freed)."""
    if path is None:
        return vectors
    from .rotation import Rotation
    return _rotated_by(Rotation.load(path), vectors)


def _rotated_by(rotation, vectors):
    rotated = rotation.rotate_word_vectors(vectors)
    if vectors.matrix is not None:
        vectors.matrix.close()
    return rotated


def _aligned(path, vectors):
    """The source vectors as read, or with -a mapped on the device by that file (the unmapped matrix is freed).
    ValueError: a map of another dimension."""
    if path is None:
        return vectors
    from .rotation import Rotation
    rotation = Rotation.load(path)
    if rotation.dimension != vectors.dimension:
        raise ValueError(f"{path}: a map of dimension {rotation.dimension} for source vectors of dimension "
                         f"{vectors.dimension}")
    return _rotated_by(rotation, vectors)


def _parser():
    p = argparse.ArgumentParser(prog="python -m gulon_amd",
                                description="build and query a Gulon nearest neighbour index")
    sub = p.add_subparsers(dest="command", required=True)
    b = sub.add_parser("build-index", help="build a nearest neighbour index",
                       description="build a nearest neighbour index")
    b.add_argument("-d", "--metric", type=_metric, required=True, metavar="l2,cosine", help="distance metric to use")
    b.add_argument("-k", "--clusters", type=_clusters, default=256, metavar="num_clusters",
                   help="clusters per quantizer, between 1 and 65536")
    b.add_argument("-m", "--quantizers", type=_integer, default=25, metavar="num", help="number of quantizers used")
    b.add_argument("-n", "--max-iters", type=_integer, default=100, metavar="iterations",
                   help="maximum number of iterations per quantizer")
    b.add_argument("-p", "--partitioned", action="store_true", help="enable faster queries by partitioning vectors")
    b.add_argument("--partitions", type=_integer, default=None, metavar="num", help="set fixed number of partitions")
    b.add_argument("-l", "--limit", type=_integer, default=None, metavar="num", help="number of partitions to search")
    b.add_argument("-o", "--output", required=True, metavar="file", help="index output file")
    b.add_argument("-R", "--rotation", default=None, metavar="file",
                   help="learn an orthogonal rotation on the vectors as read, write it to this file and build the index "
                        "over the rotated vectors; with --partitioned too the rotation is learned for the flat quantizer, "
                        "not for the partitions' residuals")
    b.add_argument("--rotation-rounds", type=_rounds, default=None, metavar="num",
                   help="refinement rounds after the initial rotation (needs --rotation; default 4)")
    b.add_argument("file", metavar="file")
    bf = sub.add_parser("build-fine", help="build the fine index of a nearest neighbour index",
                        description="build the fine index of a nearest neighbour index: a second quantizer over the "
                                    "residuals the index leaves")
    bf.add_argument("-i", "--index", required=True, metavar="file", help="path to ANN index")
    bf.add_argument("-v", "--vectors", required=True, metavar="file",
                    help="word2vec word vectors the index was built from")
    bf.add_argument("-k", "--clusters", type=_clusters, default=256, metavar="num_clusters",
                    help="clusters per quantizer, between 1 and 65536")
    bf.add_argument("-m", "--quantizers", type=_integer, default=25, metavar="num", help="number of quantizers used")
    bf.add_argument("-n", "--max-iters", type=_integer, default=100, metavar="iterations",
                    help="maximum number of iterations per quantizer")
    bf.add_argument("-o", "--output", required=True, metavar="file", help="fine index output file")
    bf.add_argument("-R", "--rotation", default=None, metavar="file", help=_ROTATED_VECTORS)
    for name, help_, need_file in (("query-words", "query nearest neighbour index by word", False),
                                   ("query", "query nearest neighbour index", True)):
        s = sub.add_parser(name, help=help_, description=help_)
        s.add_argument("-k", "--neighbours", type=_positive, default=1, metavar="num",
                       help="number of nearest neighbours to return")
        s.add_argument("-i", "--index", required=True, metavar="file", help="path to ANN index")
        s.add_argument("-v", "--vectors", default=None, metavar="file",
                       help="word2vec word vectors the index was built from: re-rank the index's candidates by their "
                            "exact distance to these")
        s.add_argument("-c", "--candidates", type=_positive, default=None, metavar="num",
                       help="candidates taken from the index per query before re-ranking (needs --vectors or --fine; "
                            "default 10 * neighbours)")
        s.add_argument("-f", "--fine", default=None, metavar="file",
                       help="fine index of the index (build-fine): re-rank the index's candidates by their distance to "
                            "the two-level reconstruction")
        s.add_argument("-r", "--restrict", default=None, metavar="file",
                       help="take the neighbours from the words of this file only (one word per line; words the index "
                            "lacks are ignored and counted on stderr)")
        s.add_argument("-R", "--rotation", default=None, metavar="file",
                       help="rotation file the index was built with (build-index -R): query vectors, and the vectors of "
                            "--vectors, are rotated before they reach the index")
        s.add_argument("--exact", action="store_true",
                       help="with --vectors: the exact neighbours among the original vectors, by brute force on the "
                            "device, instead of re-ranked candidates (not with -c, -f, -r, -x or -R)")
        if name == "query-words":
            s.add_argument("-x", "--expressions", action="store_true",
                           help="read every line as an expression `word (+|- word)*` (operators as stand-alone tokens): "
                                "query with the sum of the words' vectors and leave the words themselves out of the "
                                "answer")
            s.add_argument("--method", choices=("add", "mul"), default="add",
                           help="with -x: add ranks by the distance to the sum of the words' vectors (3CosAdd), mul by "
                                "the multiplicative objective 3CosMul, the similarities to the + words over those to "
                                "the - words (a cosine index; not with -v, -f, -r or -R)")
        s.add_argument("file", nargs=None if need_file else "?", metavar="file")
    t = sub.add_parser("test", help="calculate recall of index", description="calculate recall of index")
    t.add_argument("-v", "--vectors", required=True, metavar="file", help="word2vec word vectors")
    t.add_argument("-i", "--index", required=True, metavar="file", help="path to ANN index")
    t.add_argument("-s", "--sample", type=_sample_size, default=1000, metavar="size",
                   help="number of queries to sample for recall calculation")
    t.add_argument("-e", "--error", type=_epsilon, default=0.0, metavar="relative error",
                   help="amount of relative error allowed when calculating recall")
    t.add_argument("-c", "--candidates", type=_positive, default=None, metavar="num",
                   help="report the recall of the index refined against the vectors: num candidates per query re-ranked "
                        "by exact distance.  Each R@k is a prefix of ONE refined result per query, over "
                        "max(num, largest k) candidates, not a refined query at that k")
    t.add_argument("-f", "--fine", default=None, metavar="file",
                   help="report the recall of the index refined against this fine index (build-fine) instead of the "
                        "vectors; needs --candidates")
    t.add_argument("-R", "--rotation", default=None, metavar="file", help=_ROTATED_VECTORS)
    i = sub.add_parser("inspect", help="report code usage and quantization error of an index",
                       description="report code usage and quantization error of an index")
    i.add_argument("-i", "--index", required=True, metavar="file", help="path to ANN index")
    i.add_argument("-v", "--vectors", default=None, metavar="file",
                   help="word2vec word vectors the index was built from: report the error of the index's rows "
                        "against these")
    i.add_argument("-w", "--worst", type=_positive, default=None, metavar="num",
                   help="words with the largest error to list (needs --vectors; default 10)")
    i.add_argument("-R", "--rotation", default=None, metavar="file", help=_ROTATED_VECTORS + " (needs --vectors)")
    a = sub.add_parser("analogies", help="report the analogy accuracy of an index",
                       description="report the a:b :: c:d accuracy of an index on a questions-words.txt file: one line "
                                   "per section and a total")
    a.add_argument("-i", "--index", required=True, metavar="file", help="path to ANN index")
    a.add_argument("-k", "--depths", type=_depths, default=(1, 5, 10), metavar="k1,k2,...",
                   help="a question counts at k when its answer is among the first k neighbours (default 1,5,10)")
    a.add_argument("--lowercase", action="store_true", help="lower the words of the questions")
    a.add_argument("-v", "--vectors", default=None, metavar="file",
                   help="word2vec word vectors the index was built from: evaluate the index refined against these")
    a.add_argument("--exact", action="store_true",
                   help="with --vectors: evaluate the original vectors themselves, by brute force on the device")
    a.add_argument("-c", "--candidates", type=_positive, default=None, metavar="num",
                   help="candidates taken from the index per question before re-ranking (needs --vectors, not with "
                        "--exact; default 10 * the largest depth).  Not for a rotated index: this command takes no "
                        "rotation file")
    a.add_argument("--method", choices=("add", "mul"), default="add",
                   help="add asks for the neighbours of b - a + c (3CosAdd); mul ranks by the multiplicative objective "
                        "3CosMul, cos(d, b) * cos(d, c) / (cos(d, a) + 0.001) with the cosines shifted into [0, 1] (a "
                        "cosine index; with --vectors only together with --exact)")
    a.add_argument("file", metavar="file", help="questions: `: section` lines and lines of `a b c d`")
    s = sub.add_parser("similarity", help="report the word-pair rank correlation of an index",
                       description="report Spearman's rank correlation between the human scores of a word-pair "
                                   "similarity file and the index's distances: one line per section and a total")
    s.add_argument("-i", "--index", required=True, metavar="file", help="path to ANN index")
    s.add_argument("--lowercase", action="store_true", help="lower the words of the pairs")
    s.add_argument("-v", "--vectors", default=None, metavar="file",
                   help="word2vec word vectors the index was built from (needs --exact)")
    s.add_argument("--exact", action="store_true",
                   help="with --vectors: evaluate the original vectors of the index's words instead of its rows")
    s.add_argument("file", metavar="file", help="pairs: `: section` lines and lines of `word1 word2 score`")
    tr = sub.add_parser("translate", help="translate words between two aligned embedding spaces",
                        description="translate the words of a source embedding file into the words of a target index, "
                                    "by nearest neighbours or by CSLS; with --evaluate, report the precision of a "
                                    "bilingual dictionary")
    tr.add_argument("-i", "--index", required=True, metavar="file", help="path to the ANN index of the target language")
    tr.add_argument("-s", "--source", required=True, metavar="file",
                    help="word2vec word vectors of the source language, mapped into the target's space")
    tr.add_argument("--method", choices=("nn", "csls", "isf"), default="nn",
                    help="nn ranks by the index's distance; csls adds the mean similarity of every target word to its "
                         "nearest source words (a cosine index); isf, the inverted softmax, adds (2 / beta) times the "
                         "log of the sum of exp(-(beta / 2) * distance) over all source words (a cosine index)")
    tr.add_argument("--beta", type=_positive_float, default=None, metavar="num",
                    help="with --method isf: the inverse temperature of the inverted softmax (default 30)")
    tr.add_argument("--isf-sources", type=_positive, default=None, metavar="num",
                    help="with --method isf: normalise over the num most frequent source words only, the first num lines of "
                         "the source file (default: all)")
    tr.add_argument("-n", "--csls-neighbours", type=_positive, default=10, metavar="num",
                    help="neighbours behind the mean similarities of csls (default 10)")
    tr.add_argument("-k", "--neighbours", default=None, metavar="num",
                    help="translations printed per word (default 10); with --evaluate the depths reported, ascending and "
                         "separated by commas (default 1,5,10)")
    tr.add_argument("-e", "--evaluate", default=None, metavar="file",
                    help="a dictionary, lines of `source target`: print its precision instead of translations")
    tr.add_argument("--ranks", action="store_true",
                    help="with --evaluate: a second line with the mean reciprocal rank, the median and mean rank of the "
                         "best gold translation and the precision at the depths of -k, which may then exceed 63 (not "
                         "on an index built with -p)")
    tr.add_argument("-v", "--vectors", default=None, metavar="file",
                    help="word2vec word vectors the index was built from (needs --exact)")
    tr.add_argument("--exact", action="store_true",
                    help="with --vectors: translate into the original vectors of the index's words instead of its rows")
    tr.add_argument("-R", "--rotation", default=None, metavar="file",
                    help="rotation file the index was built with (build-index -R): the source vectors are rotated after "
                         "they are read (not with --exact)")
    tr.add_argument("-a", "--alignment", default=None, metavar="file",
                    help="map written by align: the source vectors are not mapped yet, and are mapped on the device "
                         "after they are read (before --rotation applies)")
    tr.add_argument("--lowercase", action="store_true", help="lower the words to translate")
    tr.add_argument("file", nargs="?", metavar="file", help="source words, one per line")
    al = sub.add_parser("align", help="learn the map between two embedding spaces",
                        description="learn the orthogonal map that takes the source language's word vectors into the "
                                    "target's space: a Procrustes solve on a seed dictionary, refined on CSLS mutual "
                                    "nearest neighbours")
    al.add_argument("-s", "--source", required=True, metavar="file",
                    help="word2vec word vectors of the source language, most frequent word first")
    al.add_argument("-t", "--target", required=True, metavar="file",
                    help="word2vec word vectors of the target language, most frequent word first")
    al.add_argument("-d", "--dictionary", default=None, metavar="file",
                    help="the seed dictionary, lines of `source target`")
    al.add_argument("--identical", action="store_true",
                    help="seed from the words spelt the same on both sides instead of a dictionary")
    al.add_argument("-o", "--output", required=True, metavar="file", help="map output file")
    al.add_argument("--rounds", type=_rounds, default=5, metavar="num", help="refinement rounds (default 5)")
    al.add_argument("--max-rank", type=_positive, default=15000, metavar="num",
                    help="most frequent words of either side that take part in the refinement (default 15000)")
    al.add_argument("-n", "--csls-neighbours", type=_positive, default=10, metavar="num",
                    help="neighbours behind the mean similarities of csls (default 10)")
    al.add_argument("--lowercase", action="store_true", help="lower the words of the dictionary")
    u = sub.add_parser("update", help="add, replace and remove words of an index without retraining",
                       description="add, replace and remove words of an index without retraining")
    u.add_argument("-i", "--index", required=True, metavar="file", help="path to ANN index")
    u.add_argument("-o", "--output", required=True, metavar="file", help="index output file")
    u.add_argument("-a", "--add", default=None, metavar="file",
                   help="word2vec word vectors to add; a word the index already has is replaced")
    u.add_argument("-x", "--remove", default=None, metavar="file",
                   help="words to remove, one per line (words the index lacks are ignored and counted)")
    u.add_argument("-R", "--rotation", default=None, metavar="file", help=_ROTATED_VECTORS + " (needs --add)")
    return p


def _line(word, result):
    return f"{word}: not found" if result is None else f"{word}: {','.join(result.words)}"


def query_words(index, k, lines, write):
    for s in range(0, len(lines), CHUNK):
        part = lines[s:s + CHUNK]
        for word, result in zip(part, index.batch_query_by_words(k, part)):
            write(_line(word, result) + "\n")


def query_expressions(index, k, lines, write, method="add"):
    """query-words -x: every line an expression; invalid lines are answered without reaching the index.  method "mul":
    the index's batch_query_cosmul answers in the place of batch_query_expressions."""
    from .expressions import parse_expression
    for s in range(0, len(lines), CHUNK):
        part = lines[s:s + CHUNK]
        parsed = []
        for line in part:
            try:
                parsed.append(parse_expression(line))
            except ValueError:
                parsed.append(None)
        ask = index.batch_query_cosmul if method == "mul" else index.batch_query_expressions
        results = iter(ask(k, [e for e in parsed if e is not None]))
        for line, e in zip(part, parsed):
            write((f"{line}: invalid expression" if e is None else _line(line, next(results))) + "\n")


def query(index, k, vectors, write):
    results = index.batch_query(k, vectors.data) if vectors.size else []
    for word, result in zip(vectors.words, results):
        write(_line(word, result) + "\n")


def build_config(parser, args):
    """The parsed build-index arguments as BuildIndex.Config (BuildIndex.scala:52-61 for the partitioning options)."""
    from .build import Partitioned
    if args.partitioned:
        partitioned = Partitioned(args.partitions, args.limit)
    elif args.partitions is None and args.limit is None:
        partitioned = None
    else:
        parser.error("--partitions and --limit are only applicable with --partitioned")
    if args.rotation is None:
        if args.rotation_rounds is not None:
            parser.error("--rotation-rounds is only applicable with --rotation")
        return BuildConfig(args.metric, args.clusters, args.quantizers, args.max_iters, partitioned, args.output, args.file)
    return BuildConfig(args.metric, args.clusters, args.quantizers, args.max_iters, partitioned, args.output, args.file,
                       args.rotation, args.rotation_rounds if args.rotation_rounds is not None else 4)


def run_build_index(config: BuildConfig, write):
    """BuildIndex.run (BuildIndex.scala:110-121): read (normalised for cosine), build, write."""
    from .build import build_index, log_task
    from .index_file import dump_index
    from .product_quantizer import Config
    from .word_vectors import read_word2vec_device
    vectors = log_task(write, "Reading word vectors",
                       lambda: read_word2vec_device(config.input, normalize=config.metric == "cosine"),
                       lambda v: f"Read {v.size} word vectors")             # CommandUtils.scala:112-115
    pq_config = Config(config.num_clusters, config.num_quantizers, config.max_iterations)
    if config.rotation is not None:
        from .rotation import train_rotation
        rotation, _ = train_rotation(vectors.matrix, pq_config, config.rotation_rounds, write)
        log_task(write, f"Writing rotation to {config.rotation}", lambda: rotation.save(config.rotation),
                 f"Wrote rotation to {config.rotation}")
        rotated = rotation.rotate_word_vectors(vectors)
        vectors.matrix.close()
        vectors = rotated
    words, index = build_index(vectors, config.metric, config.partitioned, pq_config, write)

    def dump():                                                              # CommandUtils.writeIndex (:117-120)
        with open(config.output, "wb") as fh:
            fh.write(dump_index(index, words))
    log_task(write, f"Writing index to {config.output}", dump, f"Wrote index to {config.output}")


def run_recall(config: RecallConfig, write, load):
    """Test.run up to the result (Test.scala:47-51, CommandUtils.scala:153-164) -> {k: SummaryStats}.
    The vectors are read with normalize=False ALWAYS, for a cosine index too, as the reference does (Test.scala:48
    passes `false`): the index normalises the query itself, the recall distances are taken on the raw vectors.
    config.rotation: the vectors are rotated on the device after they are read, the normalised reading too.
    An index form that cannot answer k = 1000 fails here with the library's message; k is never clamped.
    config.candidates: the recall of RefinedIndex(index, vectors, candidates) instead.  Its vectors are what the index
    prepares its queries for -- a NORMALISED reading of the same file for a cosine index -- while the queries and the
    recall distances stay on the raw vectors.  config.fine: the recall of FineRefinedIndex(index, that fine index file,
    candidates) instead; the vectors then serve the exact neighbours only."""
    from .build import log_task
    from .tests_recall import Tests
    from .word_vectors import read_word2vec_device
    vectors = log_task(write, "Reading word vectors", lambda: read_word2vec_device(config.vectors, normalize=False),
                       lambda v: f"Read {v.size} word vectors")
    vectors = _rotated(config.rotation, vectors)
    index = load(config.index)
    raw = vectors.sorted()
    if config.fine is not None:
        index = index.fine_refined(load(config.fine), config.candidates)
    elif config.candidates is not None:
        cosine = index.metric == "cosine"
        originals = _rotated(config.rotation, read_word2vec_device(config.vectors, normalize=True)).sorted() \
            if cosine else raw
        index = index.refined(originals, config.candidates)
    tests = log_task(write, "Sampling test vectors and precomputing distances",
                     lambda: Tests.sample(raw, config.sample_size),
                     f"Sampled {config.sample_size} vectors")
    write("\u001b[36mRUNNING:\u001b[0m Calculating recall of index\n")
    return tests.recall_of(index, config.epsilon)


def print_results(recall, write):
    """Test.printResults (Test.scala:39-43): ascending k; a k that no query kept is not in the map."""
    from .tests_recall import java_float_to_string
    for k in sorted(recall):
        stats = recall[k]
        write(f"R@{k}: {java_float_to_string(stats.mean)} +/- {java_float_to_string(stats.std_dev)}\n")


def run_inspect(config: InspectConfig, load, vectors):
    """inspect between its argument handling and its lines -> inspect.IndexReport.  For a cosine index the vectors are
    read normalised: they are what the index's rows approximate."""
    index = load(config.index)
    if config.vectors is None:
        return index.inspect()
    originals = vectors(config.vectors, index.metric == "cosine")
    if config.rotation is not None:
        from .rotation import Rotation
        originals = Rotation.load(config.rotation).rotate_word_vectors(originals)
    return index.inspect(originals, config.worst)


class UpdateError(Exception):
    """What `update` reports and exits on: a grouped index file, vectors of another dimension, a word listed twice."""


def run_update(config: UpdateConfig, write, load):
    """update behind its argument handling: load, read (normalised for a cosine index), WordIndex.update, write.
    -> the updated WordIndex."""
    from .build import log_task
    from .index_file import dump_index
    from .word_vectors import read_word2vec_device
    index = log_task(write, f"Reading index from {config.index}", lambda: load(config.index),
                     lambda i: f"Read index of {i.size} words")
    add = remove = None
    if config.add is not None:
        add = log_task(write, "Reading word vectors",
                       lambda: read_word2vec_device(config.add, normalize=index.metric == "cosine"),
                       lambda v: f"Read {v.size} word vectors")
        add = _rotated(config.rotation, add)
    if config.remove is not None:
        with open(config.remove, "rb") as fh:
            remove = read_lines(fh.read())
    try:
        updated = log_task(write, "Updating index", lambda: index.update(add=add, remove=remove),
                           lambda i: f"Updated index to {i.size} words")
    except NotImplementedError as e:
        raise UpdateError(f"{config.index}: {e}")
    except ValueError as e:
        raise UpdateError(str(e))

    def dump():
        with open(config.output, "wb") as fh:
            fh.write(dump_index(updated.index, updated.words))
    log_task(write, f"Writing index to {config.output}", dump, f"Wrote index to {config.output}")
    return updated


def run_build_fine(config: FineConfig, write, load):
    """build-fine behind its argument handling: load the index, read the vectors (normalised for a cosine index), build
    the fine index on the device, write it."""
    from .build import log_task
    from .fine import build_fine_index
    from .index_file import dump_index
    from .product_quantizer import Config
    from .word_vectors import read_word2vec_device
    index = log_task(write, f"Reading index from {config.index}", lambda: load(config.index),
                     lambda i: f"Read index of {i.size} words")
    vectors = log_task(write, "Reading word vectors",
                       lambda: _rotated(config.rotation, read_word2vec_device(
                           config.vectors, normalize=index.metric == "cosine")).sorted(),
                       lambda v: f"Read {v.size} word vectors")
    fine = build_fine_index(index, vectors, Config(config.num_clusters, config.num_quantizers, config.max_iterations),
                            write)

    def dump():
        with open(config.output, "wb") as fh:
            fh.write(dump_index(fine.index, fine.words))
    log_task(write, f"Writing index to {config.output}", dump, f"Wrote index to {config.output}")


class AnalogiesError(Exception):
    """What `analogies` reports and exits on: an unreadable or malformed questions file, vectors that lack a word of the
    index, a depth the index form cannot answer."""


def run_analogies(config: AnalogiesConfig, load, vectors):
    """analogies between its argument handling and its lines -> analogies.AnalogyReport.  For a cosine index the vectors
    are read normalised, as the query commands read them."""
    from .analogies import evaluate_analogies, read_questions
    try:
        with open(config.questions, "rb") as fh:
            sections = read_questions(read_lines(fh.read()), config.lowercase)
    except OSError as e:
        raise AnalogiesError(f"{config.questions}: {e.strerror or e}")
    except ValueError as e:
        raise AnalogiesError(f"{config.questions}: {e}")
    index = load(config.index)
    try:
        if config.vectors is not None:
            originals = vectors(config.vectors, index.metric == "cosine")
            if config.exact:
                index = index.exact(originals)
            else:
                index = index.refined(originals, config.candidates if config.candidates is not None
                                      else 10 * config.ks[-1])
        if config.method == "add":
            return evaluate_analogies(index, sections, config.ks)
        return evaluate_analogies(index, sections, config.ks, method=config.method)
    except (LookupError, NotImplementedError, ValueError) as e:
        raise AnalogiesError(str(e))


class SimilarityError(Exception):
    """What `similarity` reports and exits on: an unreadable or malformed pairs file, vectors that lack a word of the
    index, more pairs than can be ranked."""


def run_similarity(config: SimilarityConfig, load, vectors):
    """similarity between its argument handling and its lines -> similarity.SimilarityReport.  For a cosine index the
    vectors are read normalised, as the query commands read them."""
    from .similarity import evaluate_pairs, read_pairs
    try:
        with open(config.pairs, "rb") as fh:
            sections = read_pairs(read_lines(fh.read()), config.lowercase)
    except OSError as e:
        raise SimilarityError(f"{config.pairs}: {e.strerror or e}")
    except ValueError as e:
        raise SimilarityError(f"{config.pairs}: {e}")
    index = load(config.index)
    try:
        if config.exact:
            index = index.exact(vectors(config.vectors, index.metric == "cosine"))
        return evaluate_pairs(index, sections)
    except (LookupError, NotImplementedError, ValueError) as e:
        raise SimilarityError(str(e))


class TranslateError(Exception):
    """What `translate` reports and exits on: an unreadable or malformed file, vectors of another dimension, csls on an
    index that cannot answer it."""


def _frequent_rows(count, read):
    """--isf-sources N -> the rows of the source that hold the N most frequent words.  A word2vec file lists its words
    by falling frequency and `read`, the source as its reader returned it, is in word order: sorted() left behind the
    line every row came from (file_rows), and the rows of the first N lines are returned, ascending.  A reader that
    kept the file's order leaves no file_rows, and then the first N rows are the answer: N itself.  None stays None.
    ValueError: N beyond the source's words."""
    if count is None:
        return None
    if not 1 <= count <= read.size:
        raise ValueError(f"requirement failed: --isf-sources {count} outside [1, {read.size}], the source's words")
    import numpy as np
    file_rows = getattr(read, "file_rows", None)
    return count if file_rows is None else np.flatnonzero(np.asarray(file_rows) < count).astype(np.int32)


def _ranked_evaluation(index, source, pairs, config, sources=None):
    """translate -e --ranks -> ranks.RankReport whose lines are the precision line and the line of rank statistics.  The
    ranks come first, so an index that has no rank queries is refused before anything is evaluated.  csls: the rank IS
    the position in the offset query's answer, so the precision line is counted from the ranks -- the numbers
    evaluate_dictionary gives, at any depth and without selecting a list.  nn: the precision line is
    evaluate_dictionary's, in the tie order of the ordinary query; the ranks order equal distances by row."""
    from .csls import TranslationReport, evaluate_dictionary
    from .ranks import evaluate_dictionary_ranks
    report = evaluate_dictionary_ranks(index, source, pairs, config.ks, config.method, config.neighbours, config.beta,
                                       sources)
    if config.method in ("csls", "isf"):
        report.precision_report = TranslationReport(report.ks, config.method, report.asked, report.skipped,
                                                    {k: report.hits(k) for k in report.ks})
    else:
        report.precision_report = evaluate_dictionary(index, source, pairs, config.ks, config.method, config.neighbours)
    return report


def run_translate(config: TranslateConfig, write, load, vectors):
    """translate between its argument handling and the end of its output: the translations are written as they come;
    with a dictionary -> csls.TranslationReport, else None.  The source vectors are read as the index's own were: in
    word order, normalised for a cosine index.  config.beta and config.isf_sources are read for --method isf only (nn
    and csls never use them; a plain TranslateConfig carries their defaults), and --isf-sources counts in FILE order:
    _frequent_rows turns it into the rows of the most frequent words."""
    from .csls import evaluate_dictionary, read_dictionary, translate_words
    from .exact import ExactIndex, ExactWordIndex
    path = config.dictionary if config.dictionary is not None else config.words
    try:
        with open(path, "rb") as fh:
            lines = read_lines(fh.read())
        pairs = read_dictionary(lines, config.lowercase) if config.dictionary is not None else None
    except OSError as e:
        raise TranslateError(f"{path}: {e.strerror or e}")
    except ValueError as e:
        raise TranslateError(f"{path}: {e}")
    index = load(config.index)
    try:
        cosine = index.metric == "cosine"
        if config.exact:
            index = index.exact(vectors(config.vectors, cosine))
        try:
            read = vectors(config.source, cosine)
            sources = _frequent_rows(config.isf_sources, read)       # before -a and -R wrap the vectors: rows stay rows
            originals = _aligned(config.alignment, read)
        except OSError as e:
            raise TranslateError(f"{config.alignment}: {e.strerror or e}")
        originals = _rotated(config.rotation, originals)
        source = ExactWordIndex(originals.words, ExactIndex(originals.matrix, index.metric), originals.key_index)
        if pairs is not None and config.ranks:
            return _ranked_evaluation(index, source, pairs, config, sources)
        if pairs is not None:
            return evaluate_dictionary(index, source, pairs, config.ks, config.method, config.neighbours, config.beta,
                                       sources)
        words = [w.lower() for w in lines] if config.lowercase else lines
        offsets = None
        if words:                                                # the offsets once, for every chunk of words
            from .csls import method_offsets
            offsets = method_offsets(index, source, config.method, config.neighbours, config.beta, sources)
        try:
            for s in range(0, len(words), CHUNK):
                part = words[s:s + CHUNK]
                results = translate_words(index, source, part, config.k, config.method, config.neighbours, offsets)
                for word, result in zip(lines[s:s + CHUNK], results):
                    write(_line(word, result) + "\n")
        finally:
            if offsets is not None:
                offsets.free()
        return None
    except (LookupError, NotImplementedError, ValueError) as e:
        raise TranslateError(str(e))


class AlignError(Exception):
    """What `align` reports and exits on: an unreadable or malformed file, vectors of different dimensions, a seed
    without a usable pair."""


def read_ranked(path):
    """The vectors of align: on the device, normalised, in FILE order -- the row is the frequency rank."""
    from .word_vectors import read_word2vec_device
    return read_word2vec_device(path, normalize=True)


def run_align(config: AlignConfig, write, vectors=None):
    """align between its argument handling and the end of its output: the seed, the rounds and the choice are written
    as lines, the map to config.output.  vectors: path -> DeviceWordVectors in file order (default read_ranked).
    -> (Rotation, history) of alignment.train_alignment."""
    from .alignment import identical_pairs, train_alignment
    from .csls import read_dictionary
    path = config.dictionary
    try:
        pairs = None
        if path is not None:
            with open(path, "rb") as fh:
                pairs = read_dictionary(read_lines(fh.read()), config.lowercase)
        read = vectors if vectors is not None else read_ranked
        path = config.source
        source = read(path)
        path = config.target
        target = read(path)
    except OSError as e:
        raise AlignError(f"{path}: {e.strerror or e}")
    except ValueError as e:
        raise AlignError(f"{path}: {e}")
    try:
        if pairs is None:
            pairs = identical_pairs(source, target)
        rotation, history = train_alignment(source, target, pairs, config.rounds, config.max_rank, config.neighbours)
    except ValueError as e:
        raise AlignError(str(e))
    write(f"seed: {history['seed']['used']} pairs, skipped {history['seed']['skipped']}\n")
    for t, r in enumerate(history["rounds"]):
        write(f"round {t}: mutual {r['mutual']} of {r['asked']}, criterion {r['criterion']:.6f}\n")
    write(f"chosen: round {history['chosen']}\n")
    try:
        rotation.save(config.output)
    except OSError as e:
        raise AlignError(f"{config.output}: {e.strerror or e}")
    return rotation, history


def read_originals(path, normalize):
    """The -v vectors of the query commands: on the device, in word order (their key index resolves the index's words)."""
    from .word_vectors import read_word2vec_device
    return read_word2vec_device(path, normalize=normalize).sorted()


def _loaded(args, load, rotation):
    """The index file of the query commands as loaded, or with -R behind its rotation: wrapped before -v, -f, -r and -x
    are applied, so each of them meets the rotated form."""
    index = load(args.index)
    if args.rotation is None:
        return index
    from .rotation import RotatedWordIndex, Rotation
    return RotatedWordIndex(index, (rotation if rotation is not None else Rotation.load)(args.rotation))


def _restricted(args, index):
    """The loaded index, or with -r its restriction to the words of that file."""
    if args.restrict is None:
        return index
    with open(args.restrict, "rb") as fh:
        words = read_lines(fh.read())
    index = index.restrict(words)
    print(f"{index.ignored} of {len(words)} restriction words are not in the index", file=sys.stderr)
    return index


def _refined(args, index, vectors, load):
    """The loaded index, or with -r its restriction, or with -v / -f its refined form; -c needs one of those.  With
    --exact: the exact index over its words and the -v vectors."""
    if args.vectors is None and args.fine is None:
        return _restricted(args, index)
    if args.exact:
        return index.exact(vectors(args.vectors, index.metric == "cosine"))
    candidates = args.candidates if args.candidates is not None else 10 * args.neighbours
    if args.fine is not None:
        return index.fine_refined(load(args.fine), candidates)
    return index.refined(vectors(args.vectors, index.metric == "cosine"), candidates)


def main(argv=None, stdin=None, stdout=None, load=None, build=None, recall=None, vectors=None, inspect=None,
         update=None, fine=None, rotation=None, analogies=None, similarity=None, translate=None, align=None):
    """Returns the exit code.  stdin / stdout: binary streams (default: the process's); load: path -> index with
    batch_query_by_words / batch_query (default WordIndex.load); build: (BuildConfig, write) -> None, the whole of
    build-index behind its argument handling (default run_build_index); recall: (RecallConfig, write, load) ->
    {k: SummaryStats}, the whole of test between its argument handling and its result lines (default run_recall);
    vectors: (path, normalize) -> the word vectors behind -v of the query commands (default read_originals); inspect:
    (InspectConfig, load, vectors) -> IndexReport, the whole of inspect between its argument handling and its lines
    (default run_inspect); update: (UpdateConfig, write, load) -> the updated index with its four counters, the whole
    of update behind its argument handling (default run_update); fine: (FineConfig, write, load) -> None, the whole of
    build-fine behind its argument handling (default run_build_fine).  The fine index behind -f is read with `load`.  rotation: path -> the rotation behind -R of the
    query commands (default Rotation.load).  analogies: (AnalogiesConfig, load, vectors) -> AnalogyReport, the whole of
    analogies between its argument handling and its lines (default run_analogies).  similarity: (SimilarityConfig, load,
    vectors) -> SimilarityReport, the same for similarity (default run_similarity).  translate: (TranslateConfig, write,
    load, vectors) -> TranslationReport or None, the whole of translate behind its argument handling (default
    run_translate).  align: (AlignConfig, write) -> anything, the whole of align behind its argument handling
    (default run_align)."""
    parser = _parser()
    args = parser.parse_args(argv)
    if args.command == "similarity":
        if args.exact and args.vectors is None:
            parser.error("--exact needs -v/--vectors")
        if args.vectors is not None and not args.exact:
            parser.error("--vectors is only applicable with --exact")
    if args.command == "translate":
        if (args.file is None) == (args.evaluate is None):
            parser.error("exactly one of a file of words and -e/--evaluate is required")
        if args.exact and args.vectors is None:
            parser.error("--exact needs -v/--vectors")
        if args.vectors is not None and not args.exact:
            parser.error("--vectors is only applicable with --exact")
        if args.ranks and args.evaluate is None:
            parser.error("--ranks is only applicable with -e/--evaluate")
        if args.beta is not None and args.method != "isf":
            parser.error("--beta is only applicable with --method isf")
        if args.isf_sources is not None and args.method != "isf":
            parser.error("--isf-sources is only applicable with --method isf")
        if args.exact and args.rotation is not None:
            parser.error("--exact is not applicable with -R/--rotation")
        try:
            depth = _depths(args.neighbours or "1,5,10") if args.evaluate is not None \
                else _positive(args.neighbours or "10")
        except argparse.ArgumentTypeError as e:
            parser.error(f"argument -k/--neighbours: {e}")
    if args.command == "align" and (args.dictionary is None) != args.identical:
        parser.error("exactly one of -d/--dictionary and --identical is required")
    if args.command == "analogies":
        if args.exact and args.vectors is None:
            parser.error("--exact needs -v/--vectors")
        if args.candidates is not None and args.vectors is None:
            parser.error("--candidates is only applicable with --vectors")
        if args.candidates is not None and args.exact:
            parser.error("--candidates is not applicable with --exact")
        if args.method == "mul" and args.vectors is not None and not args.exact:
            parser.error("--method mul is only applicable with --vectors together with --exact")
    if args.command == "query-words" and args.method == "mul":
        if not args.expressions:
            parser.error("--method mul needs -x/--expressions")
        for given, option in ((args.vectors is not None, "-v/--vectors"), (args.fine is not None, "-f/--fine"),
                              (args.restrict is not None, "-r/--restrict"), (args.rotation is not None, "-R/--rotation")):
            if given:
                parser.error(f"--method mul is not applicable with {option}")
    if args.command == "update" and args.add is None and args.remove is None:
        parser.error("at least one of --add and --remove is required")
    if args.command == "inspect" and args.worst is not None and args.vectors is None:
        parser.error("--worst is only applicable with --vectors")
    if args.command in ("query", "query-words") and args.exact:
        if args.vectors is None:
            parser.error("--exact needs -v/--vectors")
        for given, option in ((args.candidates is not None, "-c/--candidates"), (args.fine is not None, "-f/--fine"),
                              (args.restrict is not None, "-r/--restrict"),
                              (getattr(args, "expressions", False), "-x/--expressions"),
                              (args.rotation is not None, "-R/--rotation")):
            if given:
                parser.error(f"--exact is not applicable with {option}")
    if args.command in ("query", "query-words") and args.candidates is not None and args.vectors is None \
            and args.fine is None:
        parser.error("--candidates is only applicable with --vectors or --fine")
    if args.command in ("query", "query-words") and args.fine is not None:
        if args.vectors is not None:
            parser.error("--fine is not applicable with --vectors")
        if args.restrict is not None:
            parser.error("--fine is not applicable with --restrict")
    if args.command == "inspect" and args.rotation is not None and args.vectors is None:
        parser.error("--rotation is only applicable with --vectors")
    if args.command == "update" and args.rotation is not None and args.add is None:
        parser.error("--rotation is only applicable with --add")
    if args.command == "test" and args.fine is not None and args.candidates is None:
        parser.error("--fine needs --candidates")
    if args.command in ("query", "query-words") and args.restrict is not None:
        if args.vectors is not None:
            parser.error("--restrict is not applicable with --vectors")
        if getattr(args, "expressions", False):
            parser.error("--restrict is not applicable with --expressions")
    vectors = vectors if vectors is not None else read_originals
    stdin = stdin if stdin is not None else sys.stdin.buffer
    stdout = stdout if stdout is not None else sys.stdout.buffer
    if load is None:
        from .word_index import WordIndex
        load = WordIndex.load

    def write(text):
        stdout.write(text.encode("utf-8"))

    def log(text):                                  # task lines appear as the tasks run
        write(text)
        stdout.flush()

    if args.command == "build-index":
        (build if build is not None else run_build_index)(build_config(parser, args), log)
    elif args.command == "build-fine":
        config = FineConfig(args.index, args.vectors, args.output, args.clusters, args.quantizers, args.max_iters,
                            args.rotation)
        (fine if fine is not None else run_build_fine)(config, log, load)
    elif args.command == "test":
        config = RecallConfig(args.vectors, args.index, args.sample, args.error, args.candidates, args.fine,
                              args.rotation)
        print_results((recall if recall is not None else run_recall)(config, log, load), write)
    elif args.command == "inspect":
        config = InspectConfig(args.index, args.vectors, args.worst if args.worst is not None else 10, args.rotation)
        for line in (inspect if inspect is not None else run_inspect)(config, load, vectors).lines():
            write(line + "\n")
    elif args.command == "analogies":
        config = AnalogiesConfig(args.index, args.file, args.depths, args.lowercase, args.vectors, args.exact,
                                 args.candidates, args.method)
        try:
            report = (analogies if analogies is not None else run_analogies)(config, load, vectors)
        except AnalogiesError as e:
            stdout.flush()
            print(f"error: {e}", file=sys.stderr)
            return 1
        for line in report.lines():
            write(line + "\n")
    elif args.command == "similarity":
        config = SimilarityConfig(args.index, args.file, args.lowercase, args.vectors, args.exact)
        try:
            report = (similarity if similarity is not None else run_similarity)(config, load, vectors)
        except SimilarityError as e:
            stdout.flush()
            print(f"error: {e}", file=sys.stderr)
            return 1
        for line in report.lines():
            write(line + "\n")
    elif args.command == "translate":
        k, ks = (10, depth) if args.evaluate is not None else (depth, (1, 5, 10))      # -k means depths with -e
        fields = (args.index, args.source, args.file, args.evaluate, args.method, args.csls_neighbours, k, ks,
                  args.lowercase, args.vectors, args.exact, args.rotation, args.alignment, args.ranks)
        config = TranslateConfig(*fields) if args.method != "isf" else \
            IsfTranslateConfig(*fields, 30.0 if args.beta is None else args.beta, args.isf_sources)
        try:
            report = (translate if translate is not None else run_translate)(config, write, load, vectors)
        except TranslateError as e:
            stdout.flush()
            print(f"error: {e}", file=sys.stderr)
            return 1
        if report is not None:
            for line in report.lines():
                write(line + "\n")
    elif args.command == "align":
        config = AlignConfig(args.source, args.target, args.output, args.dictionary, args.identical, args.rounds,
                             args.max_rank, args.csls_neighbours, args.lowercase)
        try:
            (align if align is not None else run_align)(config, write)
        except AlignError as e:
            stdout.flush()
            print(f"error: {e}", file=sys.stderr)
            return 1
    elif args.command == "update":
        config = UpdateConfig(args.index, args.output, args.add, args.remove, args.rotation)
        try:
            u = (update if update is not None else run_update)(config, log, load)
        except UpdateError as e:
            stdout.flush()
            print(f"error: {e}", file=sys.stderr)
            return 1
        write(f"{u.added} added, {u.replaced} replaced, {u.removed} removed, {u.ignored} ignored\n")
    elif args.command == "query-words":
        index = _refined(args, _loaded(args, load, rotation), vectors, load)
        if args.file is None:
            data = stdin.read()
        else:
            with open(args.file, "rb") as fh:
                data = fh.read()
        if args.expressions and args.method == "mul":
            try:
                query_expressions(index, args.neighbours, read_lines(data), write, method="mul")
            except (NotImplementedError, ValueError) as e:
                stdout.flush()
                print(f"error: {e}", file=sys.stderr)
                return 1
        else:
            (query_expressions if args.expressions else query_words)(index, args.neighbours, read_lines(data), write)
    else:
        from .word_vectors import read_word2vec
        queries = read_word2vec(args.file)
        index = _refined(args, _loaded(args, load, rotation), vectors, load)
        query(index, args.neighbours, queries, write)
    stdout.flush()
    return 0
