"""k_mam_sm issues every lane's three gathers unconditionally: a lane with
nothing to load reads a fixed dummy address and its result is zeroed
(smash-paper_amd/csrc/mam_sm.hpp).  These cases put lanes, waves and probe
addresses where that can go wrong -- waves whose other lanes only ever issue
the dummy load, waves that refill their claim, probes next to the ends of the
index arrays, every load slot on or off in all lanes at once -- on the tiny
index (4-byte elements) and on the mid genome with 8-byte packed and plain
words, with the reads as native rows (the row DMA'd straight into LDS) and as
dense records.  Every match equals the oracle's, and smash_map_batch, which
fails on a probe outside the index, passes."""
import os

import numpy as np
import pytest

from conftest import interleaved_reads

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import smashgpu as S  # noqa: E402
import oracle as O  # noqa: E402
import synth  # noqa: E402

L = 150
MIN_LEN = 20
CAP = L - MIN_LEN + 1


def _edge_reads(oix):
    """reads cut where exact-address 16-byte probes of T, U and L8 come
    closest to the ends of the arrays, reads with bytes outside acgt, and
    homopolymers (long runs: S_EXB, bisections with a prefetch side off)"""
    T = oix.T[:oix.N]
    N = int(oix.N)
    sp = [int(x) for x in oix.startpos]
    sz = [int(x) for x in oix.sizes]
    cuts = [0,                       # the first L bases of the text
            sp[0] + sz[0] - L,       # the last L of the first forward contig
            sp[1],                   # the first L of its reverse complement
            sp[1] + sz[1] - L,       # the last L of that
            sp[-1],                  # the last contig's reverse complement: first L
            N - 1 - L,               # the last L bases of the text (before '$')
            N - L,                   # ... with the terminator
            sp[1] - 1 - L // 2]      # across a contig separator
    reads = [T[c:c + L].copy() for c in cuts]
    c = sp[0] + sz[0] // 2           # a window of plain bases from the first contig
    while not np.isin(T[c:c + L], np.frombuffer(b"acgt", np.uint8)).all():
        c += L
    mid = T[c:c + L]
    for ch in (b"n", b"z", b"`"):    # 'n' (read N -> z upstream), absent / separator bytes
        for at in (0, 19, 75, L - 1):
            r = mid.copy()
            r[at] = ch[0]
            reads.append(r)
    r = mid.copy()
    r[40:60] = ord("z")
    reads.append(r)
    for ch in b"acgtz":
        reads.append(np.full(L, ch, np.uint8))
    reads.append(np.frombuffer((b"ac" * L)[:L], np.uint8).copy())
    return np.ascontiguousarray(np.stack(reads), np.uint8)


class Subject:
    """one oracle index, its device index, the reads and the oracle's matches
    of every read (computed once, shared by the cases)"""

    def __init__(self, oix, dix, reads):
        self.oix, self.dix = oix, dix
        self.reads = np.ascontiguousarray(reads, np.uint8)
        self.edge = _edge_reads(oix)
        self._want = {}

    def want(self, read):
        k = read.tobytes()
        if k not in self._want:
            self._want[k] = self.oix.search(k, min_len=MIN_LEN)
        return self._want[k]

    def search(self, reads, layout):
        n = reads.shape[0]
        d = torch.from_numpy(np.ascontiguousarray(reads)).cuda()
        stride = L
        if layout == "rows":
            d = S.to_rows(d, L)
            stride = S.read_stride(L)
        o = torch.zeros(n * CAP, dtype=torch.int64, device="cuda")
        nn = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        # (synchronous, and fails when a probe left the index: mam.hip probe_check)
        S.check(S.lib().smash_map_batch(self.dix.h, S.SMASH_MODE_MAM, MIN_LEN, S._ptr(d), stride,
                                        None, L, n, S._ptr(o), CAP, S._ptr(nn),
                                        S.vp(torch.cuda.current_stream().cuda_stream)),
                "smash_map_batch")
        torch.cuda.synchronize()
        w = o.cpu().numpy().view(np.uint64).reshape(n, CAP)
        k = nn.cpu().numpy()
        return [S.unpack_matches(w[r], k[r]) for r in range(n)]

    def check(self, reads, layout):
        got = self.search(reads, layout)
        for r in range(reads.shape[0]):
            assert got[r] == self.want(reads[r]), (layout, r, bytes(reads[r]))


@pytest.fixture(scope="module")
def tiny(tiny_fa, tiny_ix):
    return Subject(tiny_ix, S.Index.from_fasta(tiny_fa, device=0), interleaved_reads("s150"))


@pytest.fixture(scope="module")
def mid():
    g = synth.make_genome("mid")
    T, sp, sz, names = O.text_from_contigs(g)
    oix = O.Index(T, sp, sz, names)
    old = os.environ.get("SMASH_IDX_BYTES")
    os.environ["SMASH_IDX_BYTES"] = "8"
    try:
        dix = S.Index.create(T, sp, sz, names)
    finally:
        if old is None:
            del os.environ["SMASH_IDX_BYTES"]
        else:
            os.environ["SMASH_IDX_BYTES"] = old
    assert dix.info.idx_bytes == 8 and dix.info.pos_bits == 33
    r1, r2 = synth.make_reads(g, 520, L, seed=91)
    reads = np.empty((1040, L), np.uint8)
    reads[0::2], reads[1::2] = r1, r2
    return Subject(oix, dix, S.prepare_reads(reads))


@pytest.fixture(params=["tiny", "mid-packed", "mid-plain"])
def subject(request):
    if request.param == "tiny":
        return request.getfixturevalue("tiny")
    s = request.getfixturevalue("mid")
    s.dix.pack(request.param == "mid-packed")
    assert bool(s.dix.info.pos_bits) == (request.param == "mid-packed")
    return s


@pytest.mark.parametrize("layout", ["rows", "dense"])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1025])
def test_launch_sizes(subject, layout, n):
    """1, 2: a wave whose other lanes only ever issue the dummy loads; 64:
    exactly one full wave; 65: a second wave holding one read; 1025: waves
    that refill their claim"""
    assert subject.reads.shape[0] >= n
    subject.check(subject.reads[:n], layout)


@pytest.mark.parametrize("layout", ["rows", "dense"])
def test_array_ends_bad_bytes_and_runs(subject, layout):
    subject.check(subject.edge, layout)
    # each alone too: its wave's other 63 lanes hold nothing
    for r in (0, 5, 6, len(subject.edge) - 2):
        subject.check(subject.edge[r:r + 1], layout)


@pytest.mark.parametrize("layout", ["rows", "dense"])
def test_lock_step(subject, layout):
    """the same read in all 64 lanes: every load slot is on or off in all of
    them together (no lane ever takes the dummy address while another loads)"""
    for read in (subject.reads[3], subject.edge[0], subject.edge[-3]):
        subject.check(np.repeat(read[None, :], 64, axis=0), layout)
