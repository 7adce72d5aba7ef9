"""tools/genome_cache.py -- the benchmark's hg19-shaped input, kept on disk.

tools/synth.py make_genome("hg19") and smashgpu.text_from_contigs take ~20 s
of one host thread, every run, for bytes that never change.  store() (called
by __graft_entry__.build() where there is a GPU to benchmark on) writes them
once into the user's cache directory; load() reads them back on several
threads.  The file names carry a hash of the code and the data the bytes come
from, so a change of the generator makes a new cache and never a stale one.
Without a cache, or with a damaged one, the genome is synthesized as before:
the cache only saves time.

    contigs, (T, sp, sz, names) = genome_cache.genome_text("hg19")
"""
import hashlib
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, os.path.join(ROOT, "smash-paper_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

CACHED = ("hg19",)      # the other genomes are made in a second or two


def cache_dir():
    base = os.environ.get("SMASH_CACHE_DIR")
    if not base:
        base = os.path.join(os.environ.get("XDG_CACHE_HOME") or
                            os.path.join(os.path.expanduser("~"), ".cache"), "smash-paper_amd")
    return base


def _key(kind):
    """what the cached bytes depend on: the generator, the text layout, the
    bin table hg19's lengths and gaps are read from, and numpy's generator"""
    h = hashlib.sha256(b"files v1")
    for p in (os.path.join(HERE, "synth.py"),
              os.path.join(ROOT, "smash-paper_amd", "smashgpu.py"),
              os.path.join(ROOT, "data", "bins", "50000", "bins.txt")):
        with open(p, "rb") as f:
            h.update(f.read())
    h.update(np.__version__.encode())
    return "%s-%s" % (kind, h.hexdigest()[:16])


def _paths(kind):
    stem = os.path.join(cache_dir(), "genome-" + _key(kind))
    return stem + ".json", stem + ".contigs.u8", stem + ".text.u8"


def _read(path, n, threads=8):
    """the n bytes of a file into a fresh array, on `threads` threads
    (readinto releases the GIL)"""
    if os.path.getsize(path) != n:
        raise OSError("%s: %d bytes, expected %d" % (path, os.path.getsize(path), n))
    out = np.empty(n, np.uint8)
    cuts = [n * i // threads for i in range(threads + 1)]

    def part(i):
        with open(path, "rb", buffering=0) as f:
            f.seek(cuts[i])
            v = memoryview(out)[cuts[i]:cuts[i + 1]]
            got = 0
            while got < len(v):
                k = f.readinto(v[got:got + (64 << 20)])
                if not k:
                    raise OSError("%s: short read" % path)
                got += k

    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(part, range(threads)))
    return out


def synthesize(kind):
    import smashgpu as S
    import synth
    contigs = synth.make_genome(kind)
    return contigs, S.text_from_contigs(contigs)


def load(kind):
    """(contigs, (T, sp, sz, names)) from the cache, or None"""
    meta_p, con_p, txt_p = _paths(kind)
    try:
        with open(meta_p) as f:
            m = json.load(f)
        with ThreadPoolExecutor(2) as ex:
            fc = ex.submit(_read, con_p, sum(m["lengths"]))
            ft = ex.submit(_read, txt_p, m["text_bytes"])
            G, T = fc.result(), ft.result()
    except (OSError, ValueError, KeyError):
        return None
    contigs, a = [], 0
    for name, n in zip(m["contigs"], m["lengths"]):
        contigs.append((name, G[a:a + n]))
        a += n
    return contigs, (T, np.array(m["startpos"], np.uint64), np.array(m["sizes"], np.uint64),
                     list(m["names"]))


def store(kind, force=False):
    """synthesize `kind` and write its cache (data first, the description
    last, each renamed into place); returns the description's path"""
    meta_p, con_p, txt_p = _paths(kind)
    if os.path.exists(meta_p) and not force:
        return meta_p
    os.makedirs(cache_dir(), exist_ok=True)
    for q in os.listdir(cache_dir()):       # an older generator's cache of this genome
        if q.startswith("genome-%s-" % kind):
            os.remove(os.path.join(cache_dir(), q))
    contigs, (T, sp, sz, names) = synthesize(kind)
    m = {"contigs": [n for n, _ in contigs], "lengths": [int(len(s)) for _, s in contigs],
         "text_bytes": int(len(T)), "startpos": [int(x) for x in sp],
         "sizes": [int(x) for x in sz], "names": list(names)}
    tmp = ".tmp%d" % os.getpid()
    try:
        with open(con_p + tmp, "wb") as f:
            for _, s in contigs:
                f.write(memoryview(np.ascontiguousarray(s)))
        os.replace(con_p + tmp, con_p)
        with open(txt_p + tmp, "wb") as f:
            f.write(memoryview(np.ascontiguousarray(T)))
        os.replace(txt_p + tmp, txt_p)
        with open(meta_p + tmp, "w") as f:
            json.dump(m, f)
        os.replace(meta_p + tmp, meta_p)
    except OSError:                          # (a full disk: leave nothing behind)
        for q in (con_p + tmp, txt_p + tmp, meta_p + tmp, con_p, txt_p):
            if os.path.exists(q):
                os.remove(q)
        raise
    return meta_p


def genome_text(kind):
    """(contigs, (T, sp, sz, names)) of synth.make_genome(kind), from the
    cache where there is one"""
    return (load(kind) if kind in CACHED else None) or synthesize(kind)


if __name__ == "__main__":
    print(store(sys.argv[1] if len(sys.argv) > 1 else "hg19", force="--force" in sys.argv))
