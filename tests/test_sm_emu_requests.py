"""The host emulation of k_mam_sm (tools/sm_emu) counts the probe sequence's
own requests, and nothing the device adds to schedule them: the device kernel
issues every lane's three gathers unconditionally (idle lanes read one fixed
dummy address), the emulator's lane issues its real probes only.  The values
below were recorded from the commit before the gathers became unconditional,
on the tiny index and the s150 golden reads; a change to mam_sm.hpp that moves
any of them has changed the probe sequence (or what the emulator counts), not
only how the loads are issued."""
import hashlib
import os
import sys

import numpy as np
import pytest

from conftest import interleaved_reads

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tools", "sm_emu"))
import sm_emu  # noqa: E402

# (emulator, SMASH_SM_DIRECT) -> matches digest, lane iterations (sum, digest),
# requests (all, speculative), 64-byte line transitions per array
EXPECTED = {('packed', '0'): {'iters': '2365cf623b576807',
                   'iters_sum': 196537,
                   'lines': {'bitmap': 35976,
                             'isa': 48127,
                             'kmer': 4150,
                             'lcp': 8633,
                             'records': 3600,
                             'sa': 60980,
                             'text': 68263,
                             'uniq': 6413},
                   'matches': '741113d29d81a8d7',
                   'n_matches': 3689,
                   'probes': {'bitmap': 36742,
                              'isa': 48362,
                              'kmer': 4153,
                              'lcp': 13143,
                              'records': 14400,
                              'sa': 117471,
                              'text': 90008,
                              'uniq': 11404},
                   'requests': [369740, 84932]},
 ('packed', '1'): {'iters': '2365cf623b576807',
                   'iters_sum': 196537,
                   'lines': {'bitmap': 35976,
                             'isa': 48127,
                             'kmer': 4150,
                             'lcp': 8633,
                             'records': 3000,
                             'sa': 60980,
                             'text': 68263,
                             'uniq': 6413},
                   'matches': '741113d29d81a8d7',
                   'n_matches': 3689,
                   'probes': {'bitmap': 36742,
                              'isa': 48362,
                              'kmer': 4153,
                              'lcp': 13143,
                              'records': 12000,
                              'sa': 117471,
                              'text': 90008,
                              'uniq': 11404},
                   'requests': [368540, 84932]},
 ('plain', '0'): {'iters': 'b181902de724f25d',
                  'iters_sum': 231490,
                  'lines': {'bitmap': 35976,
                            'isa': 48104,
                            'kmer': 4150,
                            'lcp': 52960,
                            'records': 3600,
                            'sa': 52380,
                            'text': 80993,
                            'uniq': 6413},
                  'matches': '741113d29d81a8d7',
                  'n_matches': 3689,
                  'probes': {'bitmap': 36742,
                             'isa': 48362,
                             'kmer': 4153,
                             'lcp': 81112,
                             'records': 14400,
                             'sa': 117438,
                             'text': 106521,
                             'uniq': 11404},
                  'requests': [459782, 94628]},
 ('plain', '1'): {'iters': 'b181902de724f25d',
                  'iters_sum': 231490,
                  'lines': {'bitmap': 35976,
                            'isa': 48104,
                            'kmer': 4150,
                            'lcp': 52960,
                            'records': 3000,
                            'sa': 52380,
                            'text': 80993,
                            'uniq': 6413},
                  'matches': '741113d29d81a8d7',
                  'n_matches': 3689,
                  'probes': {'bitmap': 36742,
                             'isa': 48362,
                             'kmer': 4153,
                             'lcp': 81112,
                             'records': 12000,
                             'sa': 117438,
                             'text': 106521,
                             'uniq': 11404},
                  'requests': [458582, 94628]},
 ('wide', '1'): {'iters': 'b181902de724f25d',
                 'iters_sum': 231490,
                 'lines': {'bitmap': 35976,
                           'isa': 48127,
                           'kmer': 4150,
                           'lcp': 52960,
                           'records': 3000,
                           'sa': 60937,
                           'text': 80993,
                           'uniq': 6413},
                 'matches': '741113d29d81a8d7',
                 'n_matches': 3689,
                 'probes': {'bitmap': 36742,
                            'isa': 48362,
                            'kmer': 4153,
                            'lcp': 81112,
                            'records': 12000,
                            'sa': 117438,
                            'text': 106521,
                            'uniq': 11404},
                 'requests': [458582, 94628]}}


def _digest(b):
    return hashlib.sha256(b).hexdigest()[:16]


def measure(e, reads):
    got, iters = e.map(reads)
    return {
        "matches": _digest(repr(got).encode()),
        "n_matches": sum(len(g) for g in got),
        "iters_sum": int(iters.sum()),
        "iters": _digest(np.ascontiguousarray(iters, np.uint32).tobytes()),
        "requests": list(e.requests),
        "lines": {k: v[1] for k, v in e.counters.items()},
        "probes": {k: v[0] for k, v in e.counters.items()},
    }


@pytest.fixture(scope="module")
def emus(tiny_ix):
    tiny_ix.accel()
    return {"plain": sm_emu.Emu(tiny_ix), "wide": sm_emu.Emu(tiny_ix, wide=True),
            "packed": sm_emu.Emu(tiny_ix, packed=True)}


@pytest.fixture(scope="module")
def s150():
    return interleaved_reads("s150")


@pytest.mark.parametrize("which,direct", sorted(EXPECTED))
def test_emulator_counts_equal_recorded(emus, s150, which, direct, monkeypatch):
    monkeypatch.setenv("SMASH_SM_DIRECT", direct)
    got = measure(emus[which], s150)
    print(which, direct, got)
    assert got == EXPECTED[(which, direct)]


if __name__ == "__main__":   # prints the table above from the current tree
    import pprint

    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "oracle"))
    import gzip
    import tempfile

    import oracle as O
    with tempfile.TemporaryDirectory() as d:
        fa = os.path.join(d, "tiny.fa")
        with gzip.open(os.path.join(os.path.dirname(__file__), "golden", "tiny.fa.gz"), "rb") as f:
            open(fa, "wb").write(f.read())
        ix = O.Index.from_fasta(fa)
    ix.accel()
    E = {"plain": sm_emu.Emu(ix), "wide": sm_emu.Emu(ix, wide=True),
         "packed": sm_emu.Emu(ix, packed=True)}
    rd = interleaved_reads("s150")
    out = {}
    for w, dct in sorted(EXPECTED):
        os.environ["SMASH_SM_DIRECT"] = dct
        out[(w, dct)] = measure(E[w], rd)
    pprint.pprint(out, width=100, sort_dicts=True)
