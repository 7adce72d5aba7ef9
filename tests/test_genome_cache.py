"""tools/genome_cache.py (no GPU): what the cache gives back is what
synth.make_genome + smashgpu.text_from_contigs make, and a damaged or missing
cache is no cache."""
import os

import numpy as np

import genome_cache as G


def _same(a, b):
    (ca, (Ta, spa, sza, na)), (cb, (Tb, spb, szb, nb)) = a, b
    assert [n for n, _ in ca] == [n for n, _ in cb]
    assert all(x.dtype == y.dtype and np.array_equal(x, y)
               for (_, x), (_, y) in zip(ca, cb))
    for x, y in ((Ta, Tb), (spa, spb), (sza, szb)):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    assert list(na) == list(nb)


def test_store_load_roundtrip(tmp_path, monkeypatch):
    monkeypatch.setenv("SMASH_CACHE_DIR", str(tmp_path / "cache"))
    assert G.load("tiny") is None                      # nothing stored yet
    meta = G.store("tiny")
    assert os.path.dirname(meta) == str(tmp_path / "cache")
    _same(G.load("tiny"), G.synthesize("tiny"))
    assert G.store("tiny") == meta                     # kept, not rewritten
    assert sorted(os.listdir(tmp_path / "cache")) == sorted(
        os.path.basename(meta)[:-5] + e for e in (".json", ".contigs.u8", ".text.u8"))


def test_damaged_cache_is_no_cache(tmp_path, monkeypatch):
    monkeypatch.setenv("SMASH_CACHE_DIR", str(tmp_path))
    meta = G.store("tiny")
    text = meta[:-5] + ".text.u8"
    with open(text, "r+b") as f:
        f.truncate(os.path.getsize(text) - 1)
    assert G.load("tiny") is None
    os.remove(meta)
    assert G.load("tiny") is None
    _same(G.genome_text("tiny"), G.synthesize("tiny"))
