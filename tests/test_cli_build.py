"""`python -m gulon_amd build-index`: argument handling (gulon_amd/cli.py, command/BuildIndex.scala:29-68) against a
stub builder, the partition defaults (BuildIndex.scala:104-105) and formatDuration (CommandUtils.scala:84-97): no GPU."""
import io

import pytest

from gulon_amd import build, cli


def _run(argv):
    seen = []
    out = io.BytesIO()
    rc = cli.main(argv, stdout=out, build=lambda config, write: seen.append(config))
    return rc, seen


def _fails(argv, capsys):
    with pytest.raises(SystemExit) as e:
        _run(argv)
    assert e.value.code == 2
    return capsys.readouterr().err


def test_defaults():
    rc, seen = _run(["build-index", "-d", "l2", "-o", "out.idx", "vectors.txt"])
    assert rc == 0 and len(seen) == 1
    c = seen[0]
    assert (c.metric, c.num_clusters, c.num_quantizers, c.max_iterations) == ("l2", 256, 25, 100)
    assert c.partitioned is None and c.output == "out.idx" and c.input == "vectors.txt"


def test_every_option_short_and_long():
    _, seen = _run(["build-index", "-d", "cosine", "-k", "16", "-m", "8", "-n", "7", "-p", "--partitions", "12", "-l", "3",
                    "-o", "o", "in"])
    c = seen[0]
    assert (c.metric, c.num_clusters, c.num_quantizers, c.max_iterations) == ("cosine", 16, 8, 7)
    assert c.partitioned == build.Partitioned(12, 3)
    _, seen = _run(["build-index", "--metric", "l2", "--clusters", "65536", "--quantizers", "2", "--max-iters", "1",
                    "--partitioned", "--limit", "9", "--output", "o", "in"])
    c = seen[0]
    assert c.num_clusters == 65536 and c.partitioned == build.Partitioned(None, 9)
    _, seen = _run(["build-index", "-d", "l2", "-p", "-o", "o", "in"])
    assert seen[0].partitioned == build.Partitioned(None, None)


def test_validation_messages(capsys):
    base = ["build-index", "-o", "o", "in"]
    assert "unsupported metric: dot" in _fails(base + ["-d", "dot"], capsys)
    assert "clusters must be at least 1" in _fails(base + ["-d", "l2", "-k", "0"], capsys)
    assert "clusters must be at least 1" in _fails(base + ["-d", "l2", "-k", "-4"], capsys)
    assert "too many clusters, must be at most 65536" in _fails(base + ["-d", "l2", "-k", "65537"], capsys)


def test_partition_options_need_partitioned(capsys):
    msg = "--partitions and --limit are only applicable with --partitioned"
    assert msg in _fails(["build-index", "-d", "l2", "-o", "o", "-l", "3", "in"], capsys)
    assert msg in _fails(["build-index", "-d", "l2", "-o", "o", "--partitions", "3", "in"], capsys)


def test_required_arguments(capsys):
    _fails(["build-index", "-o", "o", "in"], capsys)              # metric
    _fails(["build-index", "-d", "l2", "in"], capsys)             # output
    _fails(["build-index", "-d", "l2", "-o", "o"], capsys)        # input file
    _fails(["build-index", "-d", "l2", "-o", "o", "-k", "many", "in"], capsys)


@pytest.mark.parametrize("size,partitions,limit", [(4999, 4, 5), (100000, 100, 5), (1000000, 1000, 50)])
def test_partition_defaults(size, partitions, limit):
    """partitions = size / 1000 (integer division), limit = max((partitions * 0.05).toInt, 5)."""
    assert build.partition_defaults(size, build.Partitioned(None, None)) == (partitions, limit)
    assert build.partition_defaults(size, build.Partitioned(12, None)) == (12, 5)
    assert build.partition_defaults(size, build.Partitioned(None, 3)) == (partitions, 3)
    assert build.partition_defaults(size, build.Partitioned(400, 7)) == (400, 7)


@pytest.mark.parametrize("ms,text", [
    (999, "999ms"),                     # ms < 1000
    (1000, "1.0s"),                     # %.1f of 1.0
    (59999, "60.0s"),                   # still the seconds branch: 59.999 rounds to 60.0
    (60000, "1m 0ms"),                  # 1 minute, remainder 0 ms through the first branch
    (3600000, "1h 0ms"),                # 1 hour, remainder 0 ms
    (3723004, "1h 2m 3.0s"),            # the hours branch passes the remainder IN MS on: 123 004 ms = 2m, 3 004 ms
    (0, "0ms"), (1250, "1.3s"), (61500, "1m 1.5s"),
])
def test_format_duration(ms, text):
    assert build.format_duration(ms) == text


def test_log_task_lines():
    lines = []
    assert build.log_task(lines.append, "Reading word vectors", lambda: 7, lambda n: f"Read {n} word vectors") == 7
    assert lines[0] == "\u001b[36mRUNNING:\u001b[0m Reading word vectors\n"
    assert lines[1].startswith("\u001b[32mSUCCESS:\u001b[0m Read 7 word vectors in ") and lines[1].endswith("ms\n")
