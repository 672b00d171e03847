"""The batch counts words (include/ggms.h, "Batch counts words"): the C header, its Python mirror (xgnn_amd/_lib.py) and
the numbers external callers index by agree, and no word is claimed twice.  Host only."""
import os
import subprocess

import pytest

from xgnn_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYERS = (1, 2, 3, 16)
TIERS = ("HOST", "REMOTE", "LOCAL", "REPLICA")
PER_LAYER = ("COUNT_EDGES", "COUNT_SRC", "COUNT_DST")  # in word order

# one line per name: NAME value; the per-layer names as NAME(i), for every layer
PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include "ggms.h"
#define P(name, value) printf("%s %d\n", name, (int)(value))
int main(int argc, char **argv) {
  int L = atoi(argv[argc - 1]);
  P("COUNTS_WORDS", GGMS_COUNTS_WORDS(L)); P("COUNTS_SAMPLE_WORDS", GGMS_COUNTS_SAMPLE_WORDS(L));
  for (int i = 0; i < L; ++i)
    printf("COUNT_EDGES(%d) %d\nCOUNT_SRC(%d) %d\nCOUNT_DST(%d) %d\n", i, GGMS_COUNT_EDGES(i), i, GGMS_COUNT_SRC(i), i,
           GGMS_COUNT_DST(i));
  P("COUNT_INPUT", GGMS_COUNT_INPUT(L)); P("COUNT_STATUS", GGMS_COUNT_STATUS(L)); P("COUNT_MISS", GGMS_COUNT_MISS(L));
  P("COUNT_TIER_HOST", GGMS_COUNT_TIER(L, GGMS_TIER_HOST)); P("COUNT_TIER_REMOTE", GGMS_COUNT_TIER(L, GGMS_TIER_REMOTE));
  P("COUNT_TIER_LOCAL", GGMS_COUNT_TIER(L, GGMS_TIER_LOCAL)); P("COUNT_TIER_REPLICA", GGMS_COUNT_TIER(L, GGMS_TIER_REPLICA));
  P("COUNT_STAGED_HIT", GGMS_COUNT_STAGED_HIT(L)); P("COUNT_EXPANSION", GGMS_COUNT_EXPANSION(L));
  P("COUNT_LINK_FORCED", GGMS_COUNT_LINK_FORCED(L)); P("NUM_TIERS", GGMS_NUM_TIERS);
  P("QUEUE_MAX_COUNTS", GGMS_QUEUE_MAX_COUNTS); P("QUEUE_MAX_LAYERS", GGMS_QUEUE_MAX_LAYERS);
  return 0;
}
"""


@pytest.fixture(scope="module")
def header_program(tmp_path_factory):
    """the program above, built as strict C with the C compiler of the oracle's build (oracle/Makefile: CC, gcc)"""
    d = tmp_path_factory.mktemp("counts_layout")
    src, exe = str(d / "layout.c"), str(d / "layout")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=c99", "-pedantic-errors", "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "include"), "-o", exe, src])
    return exe


def from_header(exe, L):
    out = subprocess.check_output([exe, str(L)], text=True)
    return {name: int(value) for name, value in (line.split() for line in out.splitlines())}


def from_python(L):
    d = {name: getattr(_lib, name)(L) for name in ("COUNTS_WORDS", "COUNTS_SAMPLE_WORDS", "COUNT_INPUT", "COUNT_STATUS",
                                                   "COUNT_MISS", "COUNT_STAGED_HIT", "COUNT_EXPANSION",
                                                   "COUNT_LINK_FORCED")}
    d.update({f"{name}({i})": getattr(_lib, name)(i) for name in PER_LAYER for i in range(L)})
    d.update({"COUNT_TIER_" + t: _lib.COUNT_TIER(L, getattr(_lib, "TIER_" + t)) for t in TIERS})
    d.update(NUM_TIERS=len(TIERS), QUEUE_MAX_COUNTS=_lib.QUEUE_MAX_COUNTS, QUEUE_MAX_LAYERS=_lib._QL)
    return d


def by_number(L):
    """the layout as numbers: what bench.py and external callers index by"""
    per_layer = {f"{name}({i})": 3 * i + k for k, name in enumerate(PER_LAYER) for i in range(L)}
    return dict(per_layer, COUNTS_WORDS=3 * L + 8, COUNTS_SAMPLE_WORDS=3 * L + 2,
                COUNT_INPUT=3 * L, COUNT_STATUS=3 * L + 1, COUNT_MISS=3 * L + 2,
                COUNT_TIER_HOST=3 * L + 2, COUNT_TIER_REMOTE=3 * L + 3, COUNT_TIER_LOCAL=3 * L + 4,
                COUNT_TIER_REPLICA=3 * L + 5, COUNT_STAGED_HIT=3 * L + 3, COUNT_EXPANSION=3 * L + 6,
                COUNT_LINK_FORCED=3 * L + 7, NUM_TIERS=4, QUEUE_MAX_COUNTS=3 * 16 + 8, QUEUE_MAX_LAYERS=16)


@pytest.mark.parametrize("L", LAYERS)
def test_header_python_and_numbers_agree(header_program, L):
    c = from_header(header_program, L)
    assert c == from_python(L)
    assert c == by_number(L)


@pytest.mark.parametrize("L", LAYERS)
def test_no_word_claimed_twice(header_program, L):
    c = from_header(header_program, L)
    words = {}
    for name, w in c.items():
        if name.startswith("COUNT_"):
            words.setdefault(w, set()).add(name)
    shared = sorted(sorted(names) for names in words.values() if len(names) > 1)
    assert shared == [["COUNT_MISS", "COUNT_TIER_HOST"], ["COUNT_STAGED_HIT", "COUNT_TIER_REMOTE"]]
    # the names cover the array exactly: no hole, nothing past the end; the sampler's prefix ends behind the status word
    assert sorted(words) == list(range(c["COUNTS_WORDS"]))
    assert c["COUNTS_SAMPLE_WORDS"] == c["COUNT_STATUS"] + 1


def test_queue_header_holds_the_deepest_batch(header_program):
    c = from_header(header_program, 16)
    assert c["QUEUE_MAX_LAYERS"] == 16 and c["QUEUE_MAX_COUNTS"] == c["COUNTS_WORDS"]
