"""BuildIndex.buildIndex (command/BuildIndex.scala:70-108) over device-resident word vectors, and the task log of
CommandUtils (CommandUtils.scala:75-110,112-148).

Every stage runs on the device -- the ingest (word_vectors.read_word2vec_device), the coarse k-means, grouped.group,
ProductQuantizer.apply, the encode -- and the matrix is never pulled back to the host."""
import time
from dataclasses import dataclass
from typing import Optional

from .grouped import LimitGroups
from .index import Index
from .kmeans import Config as KMeansConfig
from .kmeans import KMeans
from .product_quantizer import Config as ProductQuantizerConfig
from .product_quantizer import ProductQuantizer
from .vectors import Vectors


@dataclass(frozen=True)
class Partitioned:                      # BuildIndex.Config.Partitioned (BuildIndex.scala:25-27)
    num_partitions: Optional[int] = None
    limit: Optional[int] = None


def format_duration(ms):
    """CommandUtils.formatDuration (CommandUtils.scala:84-97).  The minutes branch passes the remaining ms on, the
    hours branch too -- so 3 723 004 ms is "1h 2m 3.0s"."""
    ms = int(ms)
    if ms < 1000:
        return f"{ms}ms"
    if ms < 60 * 1000:
        tenths = (ms + 50) // 100           # %.1f of ms / 1000d: java.util.Formatter rounds the decimal half up
        return f"{tenths // 10}.{tenths % 10}s"
    if ms < 60 * 60 * 1000:
        return f"{ms // (60 * 1000)}m {format_duration(ms % (60 * 1000))}"
    return f"{ms // (60 * 60 * 1000)}h {format_duration(ms % (60 * 60 * 1000))}"


def log_task(write, start_message, task, success_message):
    """CommandUtils.logTask (CommandUtils.scala:99-110): RUNNING, the task, SUCCESS with its duration.
    success_message: a string, or a function of the task's result.  write: text -> None, or None for silence."""
    if write is not None:
        write(f"\u001b[36mRUNNING:\u001b[0m {start_message}\n")
    start = time.monotonic()
    result = task()
    ms = int((time.monotonic() - start) * 1000)
    if write is not None:
        text = success_message(result) if callable(success_message) else success_message
        write(f"\u001b[32mSUCCESS:\u001b[0m {text} in {format_duration(ms)}\n")
    return result


def partition_defaults(size, partitioned: Partitioned):
    """(partitions, limit) as BuildIndex.buildIndex chooses them (BuildIndex.scala:104-105)."""
    partitions = partitioned.num_partitions if partitioned.num_partitions is not None else size // 1000
    limit = partitioned.limit if partitioned.limit is not None else max(int(partitions * 0.05), 5)
    return partitions, limit


def _quantize(matrix, pq_config, write):                   # CommandUtils.quantizeVectors (CommandUtils.scala:144-148)
    config = ProductQuantizerConfig(pq_config.num_clusters, pq_config.num_quantizers, pq_config.max_iterations)
    return log_task(write, "Quantizing word vectors", lambda: ProductQuantizer.apply(matrix, config),
                    f"Quantized {matrix.rows} word vectors")


def build_index(vectors, metric, partitioned: Optional[Partitioned], pq_config, write=None):
    """BuildIndex.buildIndex (BuildIndex.scala:95-108).  vectors: word_vectors.DeviceWordVectors as read (already
    normalised for cosine); metric "l2" | "cosine"; pq_config: product_quantizer.Config.
    -> (the words in the index's row order, SortedIndex | GroupedIndex); index_file.dump_index writes them."""
    if metric not in ("l2", "cosine"):
        raise ValueError(f"unsupported metric: {metric}")
    if partitioned is None:                                                       # buildLinearIndex (:84-93)
        srt = vectors.sorted()
        quantizer = _quantize(srt.matrix, pq_config, write)
        index = log_task(write, f"Building index for {srt.size} word vectors",
                         lambda: Index.sorted(srt.matrix, quantizer, metric), f"Built index for {srt.size} word vectors")
        return srt.words, index
    partitions, limit = partition_defaults(vectors.size, partitioned)             # buildSublinearIndex (:70-82)
    # CommandUtils.computePartitions (:127-133): the vectors as read, KMeans.Config(partitions, maxIterations), seed 0
    clustering = log_task(write, "Computing partitions",
                          lambda: KMeans.compute_clusters(Vectors(vectors.matrix),
                                                          KMeansConfig(partitions, pq_config.max_iterations)),
                          f"Computed {partitions} partitions")
    grouped_words, gv = log_task(write, "Reindexing word vectors", lambda: vectors.grouped(clustering, gather=False),
                                 "Re-indexed word vectors")                       # groupWordVectors (:135-137)
    quantizer = _quantize(gv.residuals, pq_config, write)
    index = log_task(write, f"Building index for {gv.size} word vectors",
                     lambda: Index.grouped(gv, quantizer, LimitGroups(limit), metric),
                     f"Built index for {gv.size} word vectors")
    return grouped_words.words, index
