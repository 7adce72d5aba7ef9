"""Which blocks of k_mam_sm's loop (smash-paper_amd/csrc/mam_sm.hpp) the test
inputs reach, on the host emulation (tools/sm_emu): every consume block and
every decide block is entered, and every block is followed by each successor
its source can hand the lane to -- the next block of the decide chain, END
(the block named the next probe, or finished the read), PARK (the chain goes
backwards: one iteration in S_ALU) or A_TOPR (A_TOP through the root reset).
The emulator records them through SM_REGION and SM_HOOK_PARK.  A rewrite of
how the blocks hand values to each other is only tested where the inputs take
the hand-over, so this is the list to read beside tests/test_sm_emu.py.

Inputs: the tiny and the mid genome; test_gpu_sm_loads.py's edge reads plus a
few hundred synthetic reads; plain and packed index words; 8 linear L8 blocks
per run side (the device's) and 1 (every longer run bisects); the four filter
policies.  Every match equals the oracle's."""
import os
import sys

import numpy as np
import pytest

from conftest import interleaved_reads

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tools", "sm_emu"))
import sm_emu  # noqa: E402
from sm_emu import END, PARK, RESET  # noqa: E402

# block -> the successors its source can take (mam_sm.hpp, in chain order)
SUCCESSORS = {
    "S_ALU": ["A_TOP", RESET],
    "S_COPY": ["A_TOP"],
    "S_BM": ["A_TOP", END],                       # END: policy 0's second B-mer probe
    "S_KT": ["A_TRAV"],
    "S_IDX": ["A_TRAV", "A_AFTER", "A_BSP", "A_EXPAND", END, RESET],
    "S_BYTE": ["A_EMIT"],
    "S_CMP": [END, "A_AFTER", "A_BSP", "A_BS"],
    "S_USCAN": [END, "A_CHAIN_DONE"],
    "S_EX": ["A_XL_DONE", "A_RUN_DONE", END, "A_BS"],
    "A_BSP": ["A_BS", END],
    "A_BS": [END, "A_BS_DONE"],
    "A_BS_DONE": ["A_XL_DONE", "A_RUN_DONE", "A_AFTER", "A_EXS"],
    "A_EXPAND": ["A_EXS"],
    "A_EXS": [END, "A_RUN_DONE"],
    "A_XL_DONE": [RESET, END, "A_RUN_DONE"],
    "A_RUN_DONE": ["A_AFTER", RESET, "A_TOP"],
    "A_CHAIN_DONE": [RESET, END],
    "A_TOP": ["A_DONE", END, "A_TRAV", PARK],
    "A_TRAV": ["A_AFTER", END],
    "A_AFTER": [PARK, END, "A_EMIT"],
    "A_EMIT": [END],
    "A_DONE": [END],
}

# transitions these inputs cannot reach (at most 3), each with its reason
UNREACHED = {
    ("S_IDX", RESET):
        "O_NS_ISA2 at depth 0: A_AFTER takes a non-singleton suffix link only at depth >= 2 and "
        "decrements once, so the ISA words arrive at depth >= 1 for every input",
    ("A_AFTER", PARK):
        "depth <= 1 after a traverse (and its continuation S_ALU -> A_TOPR): needs a search from "
        "the root that agrees on at most one character, which the window filter leaves only to a "
        "window holding a non-ACGT byte of the text; no read here lands on one",
    ("S_IDX", "A_AFTER"):
        "O_SAPOS2: a singleton interval without its position at the end of the read, after an "
        "expand_link; the chains of these reads leave (B) on non-singleton intervals",
}
CONTINUATION = {("S_ALU", RESET): ("A_AFTER", PARK)}   # the same transition, one iteration later


def _lower(reads):
    lo = np.arange(256, dtype=np.uint8)
    lo[65:91] += 32
    return lo[np.where(reads == ord("N"), ord("Z"), reads).astype(np.uint8)]


@pytest.fixture(scope="module")
def subjects(tiny_ix):
    import oracle as O
    import synth
    from test_gpu_sm_loads import _edge_reads
    tiny_ix.accel()
    g = synth.make_genome("mid")
    mid = O.Index(*O.text_from_contigs(g))
    mid.accel()
    r1, r2 = synth.make_reads(g, 150, 150, seed=47)
    mr = np.empty((300, 150), np.uint8)
    mr[0::2], mr[1::2] = r1, r2
    return [(tiny_ix, np.concatenate([_edge_reads(tiny_ix), interleaved_reads("s150")[:300]])),
            (mid, np.concatenate([_edge_reads(mid), _lower(mr)]))]


def test_every_block_and_successor_is_taken(subjects, monkeypatch):
    assert len(UNREACHED) <= 3
    sm_emu.lib()
    sm_emu.paths()                                   # reset
    want = {}

    def run(ix, e, reads, lin):
        got, _ = e.map(reads, lin_blocks=lin)
        for i in range(len(reads)):
            k = (id(ix), reads[i].tobytes())
            if k not in want:
                want[k] = ix.search(k[1])
            assert got[i] == want[k], (e.packed, lin, i)

    for ix, reads in subjects:
        for packed in (False, True):
            e = sm_emu.Emu(ix, packed=packed)
            for lin in (8, 1):
                run(ix, e, reads, lin)
    ix, reads = subjects[0]
    e = sm_emu.Emu(ix)
    for bm_dual in ("0", "1", "2"):
        monkeypatch.setenv("SMASH_SM_BM_DUAL", bm_dual)
        run(ix, e, reads, 8)
    blocks, edges = sm_emu.paths()
    print(blocks)
    for k in sorted(edges):
        print(k, edges[k])
    assert set(blocks) == set(SUCCESSORS)
    assert not [b for b, n in blocks.items() if n == 0], blocks
    listed = {(b, s) for b, ss in SUCCESSORS.items() for s in ss}
    assert not set(edges) - listed, sorted(set(edges) - listed)   # a successor the table lacks
    skip = set(UNREACHED) | {k for k, v in CONTINUATION.items() if v in UNREACHED}
    missing = sorted(k for k in listed - skip if not edges.get(k))
    assert not missing, missing
    reached = sorted(k for k in skip if edges.get(k))
    assert not reached, reached                       # the list above is stale: take it off
