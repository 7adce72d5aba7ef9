"""k_mam_sm's state bodies hand values to each other through registers that
are merged where divergent blocks meet (smash-paper_amd/csrc/mam_sm.hpp: the
consume blocks, the decide chain, the selects in S_IDX and bs_decide, the
root reset at A_TOP's entry).  A merge that reads a value a lane never wrote
shows where the lanes of a wave are all in one block, or all but one idle, or
where one lane alone takes a rare path -- and only sometimes, since what the
lane reads is whatever the register held.  So every shape below runs twice in
one process, the output buffers pre-filled with different garbage, on the tiny
index (4-byte elements) and on the mid genome with 8-byte packed and plain
words, the reads as native rows and as dense records.  Every match equals the
oracle's both times, and smash_map_batch, which fails on a probe outside the
index, passes."""
import numpy as np
import pytest

from test_gpu_sm_loads import CAP, L, MIN_LEN, Subject
from test_gpu_sm_loads import mid, subject, tiny  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import smashgpu as S  # noqa: E402

GARBAGE = ((0x5A5A5A5A5A5A5A5A, 0x7F7F7F7F), (-1, 0))


def search(subj, reads, layout, fill):
    """Subject.search with the match words and counts pre-filled with `fill`"""
    n = reads.shape[0]
    d = torch.from_numpy(np.ascontiguousarray(reads)).cuda()
    stride = L
    if layout == "rows":
        d = S.to_rows(d, L)
        stride = S.read_stride(L)
    o = torch.full((n * CAP,), fill[0], dtype=torch.int64, device="cuda")
    nn = torch.full((n,), fill[1], dtype=torch.int32, device="cuda")
    S.check(S.lib().smash_map_batch(subj.dix.h, S.SMASH_MODE_MAM, MIN_LEN, S._ptr(d), stride,
                                    None, L, n, S._ptr(o), CAP, S._ptr(nn),
                                    S.vp(torch.cuda.current_stream().cuda_stream)),
            "smash_map_batch")
    torch.cuda.synchronize()
    w = o.cpu().numpy().view(np.uint64).reshape(n, CAP)
    k = nn.cpu().numpy()
    return [S.unpack_matches(w[r], k[r]) for r in range(n)]


def check_twice(subj, reads, layout):
    reads = np.ascontiguousarray(reads, np.uint8)
    want = [subj.want(reads[r]) for r in range(reads.shape[0])]
    for run, fill in enumerate(GARBAGE):
        got = search(subj, reads, layout, fill)
        for r in range(reads.shape[0]):
            assert got[r] == want[r], (layout, run, r, bytes(reads[r]))


def shapes(subj):
    """name -> reads"""
    rd = subj.reads
    one_bad = rd[:64].copy()
    one_bad[37, 75] = ord("n")      # one lane of the wave holds a non-ACGT byte
    return {
        "one-wave-one-read": np.repeat(rd[5][None, :], 64, axis=0),   # all lanes or none per block
        "one-wave-different": rd[:64],
        "second-wave-one-lane": rd[:65],                               # 63 lanes only idle
        "one-bad-byte": one_bad,
        "one-read": rd[7:8],
    }


SHAPES = ["one-wave-one-read", "one-wave-different", "second-wave-one-lane", "one-bad-byte",
          "one-read"]


@pytest.mark.parametrize("layout", ["rows", "dense"])
@pytest.mark.parametrize("shape", SHAPES)
def test_merge_shapes(subject, layout, shape):  # noqa: F811
    assert isinstance(subject, Subject)
    check_twice(subject, shapes(subject)[shape], layout)
