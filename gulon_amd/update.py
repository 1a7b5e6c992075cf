"""Index updates: add, replace and remove words of a saved index without retraining.

The reference has no mutation, so an update is stated through what it has: the updated index is the SortedIndex the
reference would hold over the merged keys and the merged EncodedMatrix, whose new columns are ProductQuantizer.encode of
the added vectors by the index's own quantizer.  `plan_update` is the host half -- which words the result has, in which
order, and where every row's code comes from; the device half is PQIndex.encode and PQIndex.merged (csrc/update.hip)."""
from dataclasses import dataclass
from typing import List

import numpy as np

from .word_vectors import _jkey


@dataclass
class UpdatePlan:
    """words: the result's words in String.compareTo order; take[p]: where row p's code comes from -- >= 0 the old
    index's row, < 0 row -1 - take[p] of the added vectors; the four counters of WordIndex.update."""
    words: List[str]
    take: np.ndarray
    added: int
    replaced: int
    removed: int
    ignored: int


def plan_update(old_words, add_words=(), remove=()):
    """Removal first (words the index lacks are ignored and counted; a word listed twice counts once), then every word of
    `add_words`: one the index still has is replaced, any other added.  The result's words are the kept and the added
    ones in String.compareTo order (UTF-16 code units: KeyIndexSorted, DeviceWordVectors.sorted).  A word twice in
    `add_words` raises ValueError."""
    old_words, add_words = list(old_words), list(add_words)
    new_at = {}
    for i, w in enumerate(add_words):
        if w in new_at:
            raise ValueError(f"word {w!r} appears twice among the added words (positions {new_at[w]} and {i})")
        new_at[w] = i
    present = set(old_words)
    drop = set(remove)
    removed = len(drop & present)
    ignored = len(drop) - removed
    kept = present - drop
    replaced = sum(w in kept for w in add_words)
    entries = [(w, r) for r, w in enumerate(old_words) if w not in drop and w not in new_at]
    entries += [(w, -1 - i) for i, w in enumerate(add_words)]
    entries.sort(key=lambda e: _jkey(e[0]))
    return UpdatePlan([w for w, _ in entries], np.asarray([t for _, t in entries], np.int32).reshape(-1),
                      len(add_words) - replaced, replaced, removed, ignored)
