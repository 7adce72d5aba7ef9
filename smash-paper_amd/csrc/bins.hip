// smash-paper_amd/csrc/bins.hip -- the designer of a variable-width bin table
// (bins.txt / gc.txt of binning.sh) from the resident map.bin and text.
//
// A varbin table is defined by mappability: every bin of a chromosome holds
// the same number of uniquely mappable start positions (bins.txt column 6).
// With w(g) = 1 iff 1 <= right(g) <= k (the rule of smash_mappability_scan;
// right(g) = map.bin byte 3 + 2g), M[c] = the unique bases of contig c:
//   * the binned contigs (h_chrom_off >= 0) share nbins by largest remainder
//     over M, one bin each first (smash_bins_apportion);
//   * contig c with B bins: r[j] = j * M / B (j = 0..B), bin 0 starts at 0,
//     bin j at the unique base of rank r[j] (0-based, ascending position), a
//     bin stops where the next starts, the last at the contig's size;
//   * per bin n_unique = r[j + 1] - r[j], and n_gc / n_acgt = the text bytes
//     c|g / a|c|g|t of its bases (the resident text is lowercase).
// All integers: nothing depends on the order of a sum.
//
// Three steps, none of which lets a block wait for another block:
//  1. count (k_bincount): one wave per tile of kBTile bases of a binned
//     contig (tiles never straddle contigs): 16-byte loads of the [left,
//     right] pairs, the odd bytes masked out and compared with k two at a
//     time, population counts; the tile's c|g and a|c|g|t bytes of the text in
//     the same pass.  2 B of map + 1 B of text per base, once.
//  2. prefix sums (hipcub) of the three tile arrays (u32 -> u64); the totals
//     per contig go to the host, which apportions and lays out the ranks.
//  3. place (k_binplace): one wave per interior boundary: bisect the tile
//     prefix for the tile holding its rank (the first whose inclusive prefix
//     exceeds it: tiles without a unique base repeat a prefix value and are
//     never chosen), re-read that tile's right bytes, find the base of the
//     remaining rank from the lanes' counts, and count the text of the tile
//     before that base, so a bin's n_gc / n_acgt are differences of
//     (tile prefix + partial tile) at its two ends.
// Every byte offset into the map and the text is 64-bit.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <numeric>

#include "common.hpp"

namespace smash {
namespace {

constexpr int kBB = 256;                     // threads per block (4 waves)
constexpr uint32_t kBTile = 4096;            // bases per tile (one wave's)
constexpr int kBSegLds = 128;                // segment tables up to this size live in LDS
constexpr uint64_t kNoPos = ~0ull;

// one binned contig: its first base among the concatenated forward contigs
// (map2 byte 2 * g0), its text position, size, and first tile
struct BSeg {
  uint64_t g0, text0, S, tile0;
};

// the segment holding tile T (segs ascending by tile0)
__device__ __forceinline__ uint32_t bseg_of(const BSeg *segs, uint32_t nseg, uint64_t T) {
  uint32_t lo = 0, hi = nseg;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (segs[mid].tile0 <= T) lo = mid;
    else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ uint4 bload16(const uint8_t *p) {
  uint4 v;
  __builtin_memcpy(&v, p, 16);
  return v;
}

// 0x8000 in each half of the result whose right byte r (the odd bytes of two
// [left, right] pairs) has 1 <= r <= k; k2 = (0x8000 | k) in both halves:
// r + 0x7FFF reaches bit 15 iff r >= 1, (0x8000 | k) - r keeps it iff r <= k,
// and neither crosses into the other half (r <= 255, k <= 254)
__device__ __forceinline__ uint32_t uniq2(uint32_t w, uint32_t k2) {
  const uint32_t x = (w >> 8) & 0x00FF00FFu;
  return (x + 0x7FFF7FFFu) & (k2 - x) & 0x80008000u;
}
__device__ __forceinline__ uint32_t uniq8_count(const uint4 &v, uint32_t k2) {
  return uint32_t(__popc(uniq2(v.x, k2)) + __popc(uniq2(v.y, k2)) + __popc(uniq2(v.z, k2)) +
                  __popc(uniq2(v.w, k2)));
}
// bit q (0..7): base q of the 8 pairs is unique
__device__ __forceinline__ uint32_t uniq8_mask(const uint4 &v, uint32_t k2) {
  uint32_t m = 0;
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) {
    const uint32_t u = uniq2(j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w, k2);
    m |= (((u >> 15) & 1u) | ((u >> 30) & 2u)) << (2 * j);
  }
  return m;
}

// 0x80 in each byte of w that is zero (exact, no borrows)
__device__ __forceinline__ uint32_t zero_bytes(uint32_t w) {
  const uint32_t nz = (((w & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | w) & 0x80808080u;
  return ~nz & 0x80808080u;
}
// 0x80 in each byte that is c|g ('c' 0x63 and 'g' 0x67 differ in bit 2 only),
// and in each that is a|c|g|t
__device__ __forceinline__ void gc4(uint32_t w, uint32_t &cg, uint32_t &acgt) {
  cg = zero_bytes((w | 0x04040404u) ^ 0x67676767u);
  acgt = cg | zero_bytes(w ^ 0x61616161u) | zero_bytes(w ^ 0x74747474u);
}
// the c|g and a|c|g|t bytes of 16 text bytes as cg | acgt << 32
__device__ __forceinline__ uint64_t gc16_count_all(const uint4 &v) {
  uint32_t ncg = 0, nac = 0;
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) {
    uint32_t cg, ac;
    gc4(j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w, cg, ac);
    ncg += uint32_t(__popc(cg));
    nac += uint32_t(__popc(ac));
  }
  return uint64_t(ncg) | (uint64_t(nac) << 32);
}

// the first nbytes of a 16-byte block whose later bytes may lie past the
// buffer: whole when all 16 are there, else byte by byte, the rest 0 (a pair
// [0, 0] is not unique, a text byte 0 is no base)
__device__ __forceinline__ uint4 bload_head(const uint8_t *p, uint32_t nbytes) {
  if (nbytes >= 16) return bload16(p);
  uint32_t w[4] = {0, 0, 0, 0};
  for (uint32_t b = 0; b < nbytes; ++b) w[b >> 2] |= uint32_t(p[b]) << (8 * (b & 3));
  return make_uint4(w[0], w[1], w[2], w[3]);
}

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// step 1: per tile the unique bases, and (text != null) the c|g and a|c|g|t
// bytes.  One wave per tile, waves dealt over the tiles with the grid's
// stride; wave-load j of the map covers bases 512 j + 8 lane .. + 8 (1 KiB
// contiguous per instruction), of the text bytes 1024 j + 16 lane .. + 16.
__global__ __launch_bounds__(kBB) void k_bincount(const uint8_t *__restrict__ map2,
                                                  const uint8_t *__restrict__ text,
                                                  const BSeg *__restrict__ segs, uint32_t nseg,
                                                  uint64_t ntiles, uint32_t k,
                                                  uint32_t *__restrict__ t_uniq,
                                                  uint32_t *__restrict__ t_gc,
                                                  uint32_t *__restrict__ t_acgt) {
  __shared__ BSeg s_segs[kBSegLds];
  const bool lds_segs = nseg <= uint32_t(kBSegLds);
  if (lds_segs)
    for (uint32_t q = threadIdx.x; q < nseg; q += blockDim.x) s_segs[q] = segs[q];
  __syncthreads();   // (the only barrier: the waves go their own ways from here)
  const BSeg *tab = lds_segs ? s_segs : segs;
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t k2 = (0x8000u | k) * 0x00010001u;
  const uint64_t waves = uint64_t(gridDim.x) * (kBB / 64);
  for (uint64_t T = uint64_t(blockIdx.x) * (kBB / 64) + (threadIdx.x >> 6); T < ntiles;
       T += waves) {
    const BSeg g = tab[bseg_of(tab, nseg, T)];
    const uint64_t tb = (T - g.tile0) * kBTile;              // the tile's first base in the contig
    const uint32_t n = uint32_t(std::min<uint64_t>(kBTile, g.S - tb));
    const uint8_t *mp = map2 + 2 * (g.g0 + tb);
    const uint8_t *tp = text ? text + g.text0 + tb : nullptr;
    uint32_t nu = 0;
    uint64_t ng = 0;
    if (n == kBTile) {   // (wave-uniform) every load whole: all twelve in flight together
      uint4 m[8], t[4];
#pragma unroll
      for (uint32_t j = 0; j < 8; ++j) m[j] = bload16(mp + 1024 * j + 16 * lane);
      if (tp) {
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) t[j] = bload16(tp + 1024 * j + 16 * lane);
      }
#pragma unroll
      for (uint32_t j = 0; j < 8; ++j) nu += uniq8_count(m[j], k2);
      if (tp) {
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) ng += gc16_count_all(t[j]);
      }
    } else {             // a contig's last tile: nothing past its n bases is read
      for (uint32_t j = 0; j < 8; ++j) {
        const uint32_t b = 512 * j + 8 * lane;
        if (b < n) nu += uniq8_count(bload_head(mp + 2 * uint64_t(b), 2 * (n - b)), k2);
      }
      if (tp) {
        for (uint32_t j = 0; j < 4; ++j) {
          const uint32_t b = 1024 * j + 16 * lane;
          if (b < n) ng += gc16_count_all(bload_head(tp + b, n - b));
        }
      }
    }
    // <= 4096 each: 16 bits apiece of one word
    const uint64_t s = wave_sum(uint64_t(nu) | ((ng & 0xFFFFu) << 16) | ((ng >> 32) << 32));
    if (lane == 0) {
      t_uniq[T] = uint32_t(s & 0xFFFFu);
      if (tp) {
        t_gc[T] = uint32_t((s >> 16) & 0xFFFFu);
        t_acgt[T] = uint32_t(s >> 32);
      }
    }
  }
}

// the prefix values at every segment's first tile and past the last one
__global__ void k_bin_segpre(const BSeg *segs, uint32_t nseg, uint64_t ntiles,
                             const uint64_t *p_uniq, const uint64_t *p_gc, const uint64_t *p_acgt,
                             uint64_t *out) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q > nseg) return;
  const uint64_t T = q < nseg ? segs[q].tile0 : ntiles;
  out[3 * q] = p_uniq[T];
  out[3 * q + 1] = p_gc ? p_gc[T] : 0;
  out[3 * q + 2] = p_acgt ? p_acgt[T] : 0;
}

// one interior boundary: the unique base of rank `rank` among all tiles'
// unique bases, known to lie in segment seg
struct BBound {
  uint64_t rank;
  uint32_t seg, pad;
};

// step 3: one wave per boundary.  out[3 b] = the base's position in its
// contig (kNoPos: no such base -- the prefix and the map disagree), out[3 b +
// 1], [3 b + 2] = the c|g and a|c|g|t bytes of all tiles' text before it.
__global__ __launch_bounds__(kBB) void k_binplace(const uint8_t *__restrict__ map2,
                                                  const uint8_t *__restrict__ text,
                                                  const BSeg *__restrict__ segs, uint32_t nseg,
                                                  uint64_t ntiles, uint32_t k,
                                                  const uint64_t *__restrict__ p_uniq,
                                                  const uint64_t *__restrict__ p_gc,
                                                  const uint64_t *__restrict__ p_acgt,
                                                  const BBound *__restrict__ bounds,
                                                  uint64_t nbounds, uint64_t *__restrict__ out) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t k2 = (0x8000u | k) * 0x00010001u;
  const uint64_t waves = uint64_t(gridDim.x) * (kBB / 64);
  for (uint64_t b = uint64_t(blockIdx.x) * (kBB / 64) + (threadIdx.x >> 6); b < nbounds;
       b += waves) {
    const BBound bd = bounds[b];
    if (bd.seg >= nseg) {
      if (lane == 0) out[3 * b] = kNoPos;
      continue;
    }
    const BSeg g = segs[bd.seg];
    const uint64_t tend = bd.seg + 1 < nseg ? segs[bd.seg + 1].tile0 : ntiles;
    // the last tile T of the segment with p_uniq[T] <= rank: its inclusive
    // prefix p_uniq[T + 1] is the first to exceed the rank, so it holds a
    // unique base (a tile without one repeats the prefix and is passed over)
    uint64_t lo = g.tile0, hi = tend;   // p_uniq[lo] <= rank; answer in [lo, hi)
    while (hi - lo > 1) {
      const uint64_t mid = (lo + hi) >> 1;
      if (p_uniq[mid] <= bd.rank) lo = mid;
      else hi = mid;
    }
    const uint64_t T = lo;
    if (T >= tend) {   // (a segment without tiles has no boundary)
      if (lane == 0) out[3 * b] = kNoPos;
      continue;
    }
    const uint64_t base = p_uniq[T];
    uint64_t q = bd.rank >= base ? bd.rank - base : kNoPos;   // the rank within the tile
    const uint64_t tb = (T - g.tile0) * kBTile;
    const uint32_t n = uint32_t(std::min<uint64_t>(kBTile, g.S - tb));
    const uint8_t *mp = map2 + 2 * (g.g0 + tb);
    // four steps of 1024 bases, lane l the 16 bases 1024 c + 16 l .. in order
    uint32_t found = kBTile;   // the base's offset in the tile
    for (uint32_t c = 0; c < kBTile / 1024 && found == kBTile && q != kNoPos; ++c) {
      const uint32_t b0 = 1024 * c + 16 * lane;
      uint32_t m = 0;
      if (b0 < n) {
        m = uniq8_mask(bload_head(mp + 2 * uint64_t(b0), 2 * (n - b0)), k2);
        if (b0 + 8 < n)
          m |= uniq8_mask(bload_head(mp + 2 * uint64_t(b0) + 16, 2 * (n - b0 - 8)), k2) << 8;
      }
      const uint32_t cnt = uint32_t(__popc(m));
      uint32_t incl = cnt;   // inclusive prefix over the lanes
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(incl, d, 64);
        if (lane >= uint32_t(d)) incl += y;
      }
      const uint32_t tot = __shfl(incl, 63, 64);
      if (q < tot) {
        const uint32_t excl = incl - cnt;
        const bool mine = q >= excl && q < incl;   // exactly one lane
        uint32_t pos = 0;
        if (mine) {
          uint32_t mm = m;
          for (uint32_t r = uint32_t(q) - excl; r; --r) mm &= mm - 1;
          pos = b0 + uint32_t(__builtin_ctz(mm));
        }
        const uint64_t who = __ballot(mine);
        found = __shfl(pos, who ? int(__builtin_ctzll(who)) : 0, 64);
      } else {
        q -= tot;
      }
    }
    if (found >= n) {   // (kBTile: not found)
      if (lane == 0) out[3 * b] = kNoPos;
      continue;
    }
    // the text of the tile before the base
    uint64_t ng = 0;
    if (text) {
      const uint8_t *tp = text + g.text0 + tb;
      for (uint32_t c = 0; c < kBTile / 1024; ++c) {
        const uint32_t b0 = 1024 * c + 16 * lane;
        if (b0 < found) {
          // (the bytes of this block before the base; the rest stay 0)
          ng += gc16_count_all(bload_head(tp + b0, found - b0));
        }
      }
      ng = wave_sum(ng);   // (<= 4096 per half)
    }
    if (lane == 0) {
      out[3 * b] = tb + found;
      out[3 * b + 1] = text ? p_gc[T] + (ng & 0xFFFFFFFFu) : 0;
      out[3 * b + 2] = text ? p_acgt[T] + (ng >> 32) : 0;
    }
  }
}

struct U32ToU64 {
  __host__ __device__ uint64_t operator()(uint32_t v) const { return uint64_t(v); }
};

// device buffers of one design, freed on every way out
struct Bufs {
  std::vector<void *> p;
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  template <class T>
  hipError_t get(T **out, size_t n) {
    void *q = nullptr;
    hipError_t e = hipMalloc(&q, std::max<size_t>(n, 1) * sizeof(T));
    if (e == hipSuccess) p.push_back(q);
    *out = static_cast<T *>(q);
    return e;
  }
  ~Bufs() {
    for (void *q : p) (void)hipFree(q);
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

// blocks for `waves_wanted` waves of work: no more than are resident at once
// (the occupancy query), the rest of the work by the grid's stride
unsigned bins_grid(uint64_t waves_wanted, int device, const void *kfn) {
  int cus = 0, per_cu = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess ||
      cus < 1)
    cus = 256;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kfn, kBB, 0) != hipSuccess ||
      per_cu < 1)
    per_cu = 4;
  const uint64_t blocks = (waves_wanted + kBB / 64 - 1) / (kBB / 64);
  return unsigned(std::max<uint64_t>(1, std::min<uint64_t>(blocks, uint64_t(cus) * per_cu)));
}

}  // namespace
}  // namespace smash

using namespace smash;

extern "C" uint32_t smash_bins_tile(void) { return kBTile; }

extern "C" int smash_bins_apportion(const uint64_t *h_unique, const int64_t *h_chrom_off,
                                    uint32_t n_contig, uint32_t nbins,
                                    uint32_t *h_bins_per_contig) {
  if (!h_unique || !h_chrom_off || !h_bins_per_contig) {
    set_error("smash_bins_apportion: null argument");
    return SMASH_ERR_ARG;
  }
  std::vector<uint32_t> idx;
  unsigned __int128 tot = 0;
  for (uint32_t c = 0; c < n_contig; ++c) {
    h_bins_per_contig[c] = 0;
    if (h_chrom_off[c] >= 0) {
      idx.push_back(c);
      tot += h_unique[c];
    }
  }
  if (nbins < idx.size()) {
    set_error("smash_bins_apportion: " + std::to_string(nbins) + " bins for " +
              std::to_string(idx.size()) + " binned contigs (each takes one)");
    return SMASH_ERR_ARG;
  }
  for (uint32_t c : idx) h_bins_per_contig[c] = 1;
  const uint64_t extra = nbins - idx.size();
  if (!extra) return SMASH_OK;
  if (tot == 0) {
    set_error("smash_bins_apportion: no unique base to share the bins by");
    return SMASH_ERR_ARG;
  }
  // largest remainder over extra * M / tot (the product in 128 bits); ties
  // go to the earlier contig
  std::vector<uint64_t> rem(idx.size());
  uint64_t given = 0;
  for (size_t i = 0; i < idx.size(); ++i) {
    const unsigned __int128 p = (unsigned __int128)extra * h_unique[idx[i]];
    const uint64_t q = uint64_t(p / tot);
    rem[i] = uint64_t(p % tot);
    h_bins_per_contig[idx[i]] += uint32_t(q);
    given += q;
  }
  std::vector<uint32_t> order(idx.size());
  std::iota(order.begin(), order.end(), 0u);
  std::stable_sort(order.begin(), order.end(),
                   [&](uint32_t a, uint32_t b) { return rem[a] > rem[b]; });
  for (uint64_t i = 0; i < extra - given && i < order.size(); ++i)
    h_bins_per_contig[idx[order[i]]] += 1;
  return SMASH_OK;
}

extern "C" int smash_bins_design_raw(int device, const uint8_t *d_map2, const uint8_t *d_text,
                                     uint32_t n_contig, const uint64_t *h_sizes,
                                     const uint64_t *h_text_start, const int64_t *h_chrom_off,
                                     uint32_t k, uint32_t nbins, smash_bin *h_out,
                                     uint64_t *h_contig_unique, void *stream) {
  if (!d_map2 || !h_sizes || !h_chrom_off || !h_out || (d_text && !h_text_start) || !n_contig) {
    set_error("smash_bins_design: null argument");
    return SMASH_ERR_ARG;
  }
  if (k == 0 || k > 254) {
    set_error("smash_bins_design: k must be 1..254 (a map.bin byte saturates at 255)");
    return SMASH_ERR_ARG;
  }
  // the binned contigs' segments, tiles numbered across them
  std::vector<BSeg> segs;
  std::vector<uint32_t> seg_contig;
  uint64_t g0 = 0, ntiles = 0;
  for (uint32_t c = 0; c < n_contig; ++c) {
    if (h_chrom_off[c] >= 0) {
      BSeg s;
      s.g0 = g0;
      s.text0 = d_text ? h_text_start[c] : 0;
      s.S = h_sizes[c];
      s.tile0 = ntiles;
      segs.push_back(s);
      seg_contig.push_back(c);
      ntiles += (h_sizes[c] + kBTile - 1) / kBTile;
    }
    g0 += h_sizes[c];
  }
  const uint32_t nseg = uint32_t(segs.size());
  if (nbins < nseg || nseg == 0) {
    set_error("smash_bins_design: " + std::to_string(nbins) + " bins for " + std::to_string(nseg) +
              " binned contigs (each takes one; none: nothing to bin)");
    return SMASH_ERR_ARG;
  }
  SMASH_HIP(hipSetDevice(device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool timed = getenv("SMASH_BINS_TIMES") != nullptr;   // per-step times on stderr
  Bufs B;
  if (timed)
    for (hipEvent_t &e : B.ev) SMASH_HIP(hipEventCreate(&e));
  BSeg *d_segs = nullptr;
  uint32_t *t_uniq = nullptr, *t_gc = nullptr, *t_acgt = nullptr;
  uint64_t *p_uniq = nullptr, *p_gc = nullptr, *p_acgt = nullptr, *d_segpre = nullptr;
  SMASH_HIP(B.get(&d_segs, nseg));
  SMASH_HIP(B.get(&t_uniq, ntiles + 1));
  SMASH_HIP(B.get(&p_uniq, ntiles + 1));
  if (d_text) {
    SMASH_HIP(B.get(&t_gc, ntiles + 1));
    SMASH_HIP(B.get(&t_acgt, ntiles + 1));
    SMASH_HIP(B.get(&p_gc, ntiles + 1));
    SMASH_HIP(B.get(&p_acgt, ntiles + 1));
  }
  SMASH_HIP(B.get(&d_segpre, 3 * size_t(nseg + 1)));
  SMASH_HIP(hipMemcpyAsync(d_segs, segs.data(), sizeof(BSeg) * nseg, hipMemcpyHostToDevice, s));
  // (entry ntiles of the tile arrays is the zero that turns the exclusive sums
  // over ntiles + 1 entries into the totals)
  SMASH_HIP(hipMemsetAsync(t_uniq + ntiles, 0, 4, s));
  if (d_text) {
    SMASH_HIP(hipMemsetAsync(t_gc + ntiles, 0, 4, s));
    SMASH_HIP(hipMemsetAsync(t_acgt + ntiles, 0, 4, s));
  }
  // step 1
  if (timed) SMASH_HIP(hipEventRecord(B.ev[0], s));
  if (ntiles) {
    const unsigned grid = bins_grid(ntiles, device, reinterpret_cast<const void *>(k_bincount));
    k_bincount<<<grid, kBB, 0, s>>>(d_map2, d_text, d_segs, nseg, ntiles, k, t_uniq, t_gc, t_acgt);
    SMASH_HIP(hipGetLastError());
  }
  if (timed) SMASH_HIP(hipEventRecord(B.ev[1], s));
  // step 2
  {
    size_t tmp_bytes = 0;
    hipcub::TransformInputIterator<uint64_t, U32ToU64, const uint32_t *> in(t_uniq, U32ToU64());
    SMASH_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, in, p_uniq, ntiles + 1, s));
    uint8_t *tmp = nullptr;
    SMASH_HIP(B.get(&tmp, tmp_bytes));
    SMASH_HIP(hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, in, p_uniq, ntiles + 1, s));
    if (d_text) {
      hipcub::TransformInputIterator<uint64_t, U32ToU64, const uint32_t *> ig(t_gc, U32ToU64());
      hipcub::TransformInputIterator<uint64_t, U32ToU64, const uint32_t *> ia(t_acgt, U32ToU64());
      SMASH_HIP(hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, ig, p_gc, ntiles + 1, s));
      SMASH_HIP(hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, ia, p_acgt, ntiles + 1, s));
    }
  }
  k_bin_segpre<<<(nseg + 1 + 255) / 256, 256, 0, s>>>(d_segs, nseg, ntiles, p_uniq, p_gc, p_acgt,
                                                      d_segpre);
  SMASH_HIP(hipGetLastError());
  std::vector<uint64_t> segpre(3 * size_t(nseg + 1));
  SMASH_HIP(hipMemcpyAsync(segpre.data(), d_segpre, 8 * segpre.size(), hipMemcpyDeviceToHost, s));
  if (timed) SMASH_HIP(hipEventRecord(B.ev[2], s));
  SMASH_HIP(hipStreamSynchronize(s));
  // the host's part: apportion, then every interior boundary's rank
  std::vector<uint64_t> M(n_contig, 0);
  for (uint32_t q = 0; q < nseg; ++q) M[seg_contig[q]] = segpre[3 * (q + 1)] - segpre[3 * q];
  if (h_contig_unique) std::copy(M.begin(), M.end(), h_contig_unique);
  std::vector<uint32_t> per(n_contig, 0);
  const int arc = smash_bins_apportion(M.data(), h_chrom_off, n_contig, nbins, per.data());
  if (arc != SMASH_OK) return arc;
  std::vector<BBound> bounds;
  bounds.reserve(nbins - nseg);
  for (uint32_t q = 0; q < nseg; ++q) {
    const uint32_t c = seg_contig[q];
    const uint64_t Bc = per[c], Mc = M[c];
    if (Bc > 1 && Bc > Mc) {
      set_error("smash_bins_design: contig " + std::to_string(c) + " gets " + std::to_string(Bc) +
                " bins but has " + std::to_string(Mc) + " unique positions");
      return SMASH_ERR_ARG;
    }
    for (uint64_t j = 1; j < Bc; ++j) {
      BBound b;
      b.rank = segpre[3 * q] + uint64_t((unsigned __int128)j * Mc / Bc);
      b.seg = q;
      b.pad = 0;
      bounds.push_back(b);
    }
  }
  // step 3
  std::vector<uint64_t> placed(3 * bounds.size());
  if (timed) SMASH_HIP(hipEventRecord(B.ev[3], s));
  if (!bounds.empty()) {
    BBound *d_bounds = nullptr;
    uint64_t *d_placed = nullptr;
    SMASH_HIP(B.get(&d_bounds, bounds.size()));
    SMASH_HIP(B.get(&d_placed, placed.size()));
    SMASH_HIP(hipMemcpyAsync(d_bounds, bounds.data(), sizeof(BBound) * bounds.size(),
                             hipMemcpyHostToDevice, s));
    const unsigned grid =
        bins_grid(bounds.size(), device, reinterpret_cast<const void *>(k_binplace));
    k_binplace<<<grid, kBB, 0, s>>>(d_map2, d_text, d_segs, nseg, ntiles, k, p_uniq, p_gc, p_acgt,
                                    d_bounds, bounds.size(), d_placed);
    SMASH_HIP(hipGetLastError());
    SMASH_HIP(hipMemcpyAsync(placed.data(), d_placed, 8 * placed.size(), hipMemcpyDeviceToHost, s));
  }
  if (timed) SMASH_HIP(hipEventRecord(B.ev[4], s));
  SMASH_HIP(hipStreamSynchronize(s));
  if (timed) {
    float a = 0, b = 0, c = 0;
    SMASH_HIP(hipEventElapsedTime(&a, B.ev[0], B.ev[1]));
    SMASH_HIP(hipEventElapsedTime(&b, B.ev[1], B.ev[2]));
    SMASH_HIP(hipEventElapsedTime(&c, B.ev[3], B.ev[4]));
    fprintf(stderr,
            "smash_bins_design: count %.3f ms (%llu tiles), prefix sums %.3f ms, place %.3f ms "
            "(%llu boundaries)\n",
            a, (unsigned long long)ntiles, b, c, (unsigned long long)bounds.size());
  }
  // the rows, contig by contig
  uint64_t row = 0, bi = 0;
  for (uint32_t q = 0; q < nseg; ++q) {
    const uint32_t c = seg_contig[q];
    const uint64_t Bc = per[c], Mc = M[c];
    uint64_t start = 0, gc0 = segpre[3 * q + 1], ac0 = segpre[3 * q + 2], r0 = 0;
    for (uint64_t j = 0; j < Bc; ++j, ++row) {
      uint64_t stop = h_sizes[c], gc1 = segpre[3 * (q + 1) + 1], ac1 = segpre[3 * (q + 1) + 2];
      uint64_t r1 = Mc;
      if (j + 1 < Bc) {
        stop = placed[3 * bi];
        gc1 = placed[3 * bi + 1];
        ac1 = placed[3 * bi + 2];
        r1 = uint64_t((unsigned __int128)(j + 1) * Mc / Bc);
        ++bi;
        if (stop == kNoPos || stop <= start || stop >= h_sizes[c]) {
          set_error("smash_bins_design: boundary " + std::to_string(j + 1) + " of contig " +
                    std::to_string(c) + " not found (the map changed under the design?)");
          return SMASH_ERR_HIP;
        }
      }
      smash_bin &o = h_out[row];
      o.contig = c;
      o.reserved = 0;
      o.start = start;
      o.stop = stop;
      o.abspos = h_chrom_off[c] + int64_t(start);
      o.n_unique = r1 - r0;
      o.n_gc = gc1 - gc0;
      o.n_acgt = ac1 - ac0;
      start = stop;
      gc0 = gc1;
      ac0 = ac1;
      r0 = r1;
    }
  }
  return SMASH_OK;
}

extern "C" int smash_bins_design(const smash_index *ix, const int64_t *h_chrom_off, uint32_t k,
                                 uint32_t nbins, smash_bin *h_out, uint64_t *h_contig_unique,
                                 void *stream) {
  if (!ix || !h_chrom_off || !h_out) {
    set_error("smash_bins_design: null argument");
    return SMASH_ERR_ARG;
  }
  if (!ix->rcref || !ix->d_map || ix->map_bytes < 2) {
    set_error("smash_bins_design: the index has no map.bin (it needs -rcref)");
    return SMASH_ERR_ARG;
  }
  std::vector<uint64_t> sizes, starts;
  for (uint32_t q = 0; q < ix->n_seq; q += 2) {
    sizes.push_back(ix->sizes[q]);
    starts.push_back(ix->startpos[q]);
  }
  return smash_bins_design_raw(ix->device, ix->d_map + 2, ix->d_text, uint32_t(sizes.size()),
                               sizes.data(), starts.data(), h_chrom_off, k, nbins, h_out,
                               h_contig_unique, stream);
}
