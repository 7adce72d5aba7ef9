// smash-paper_amd/csrc/verify.hip -- smash_index_verify (smash_gpu.h): a
// complete check, on the device, that the resident SA / ISA / LCP / map are
// the index of the resident text (DESIGN.md section 1 has the predicates and
// why clean counters prove the arrays).
//
// Nothing here trusts a value it has loaded: an element of SA, ISA, the LCP
// bytes or the overflow table is compared with N (or the table's size) before
// it indexes anything, x + l is tested as l >= N - x, comparison loops run to
// a length already proven to end inside the text, and a rank whose inputs are
// out of range is counted bad and skipped.  The text has 64 zero bytes past
// N; the widest load below ends 23 bytes past the last compared byte.
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>

#include "common.hpp"

namespace smash {
namespace {

// device counters (u64), copied into the report
enum : int {
  kLayoutBad, kLayoutFirst, kPermBad, kPermFirst, kOrderBad, kOrderFirst, kLcpBad, kLcpFirst,
  kOvfBad, kOvfFirst, kMapBad, kMapFirst, kN255, kIrr, kBytes, kLongest,
  kWork,      // entries appended to the work list (may exceed its capacity)
  kTicks,     // '`' bytes in the text
  kDollars,   // '$' bytes in the text
  kCounters
};

constexpr uint64_t kNone = ~0ull;
constexpr uint32_t kThreadMax = 64;       // longest comparison a thread keeps (bytes)
constexpr uint64_t kWorkCap = 1ull << 22; // work-list entries (32 B each)
constexpr uint64_t kMapWindow = 1ull << 26;

struct WorkItem {
  uint64_t rank, x, y, l;
};

struct VCtx {
  const uint8_t *T;
  const uint8_t *L8;
  const uint64_t *ovf;
  uint64_t n_ovf, N;
  unsigned long long *cnt;
  WorkItem *work;
  uint64_t work_cap;
  uint32_t flags;
};

// ---- reductions: one atomic per wave -------------------------------------
__device__ inline void flush_sum(unsigned long long *c, unsigned long long v) {
  for (int o = 32; o; o >>= 1) v += __shfl_down(v, o);
  if ((threadIdx.x & 63) == 0 && v) atomicAdd(c, v);
}
__device__ inline void flush_min(unsigned long long *c, unsigned long long v) {
  for (int o = 32; o; o >>= 1) {
    const unsigned long long w = __shfl_down(v, o);
    v = w < v ? w : v;
  }
  if ((threadIdx.x & 63) == 0 && v != kNone) atomicMin(c, v);
}
__device__ inline void flush_max(unsigned long long *c, unsigned long long v) {
  for (int o = 32; o; o >>= 1) {
    const unsigned long long w = __shfl_down(v, o);
    v = w > v ? w : v;
  }
  if ((threadIdx.x & 63) == 0 && v) atomicMax(c, v);
}

// ---- text bytes at any alignment ------------------------------------------
// 8 / 16 bytes from text position p (little endian: byte p in the low bits)
// out of aligned 8-byte words; reads at most 15 / 23 bytes past p
__device__ inline uint64_t load8(const uint8_t *T, uint64_t p) {
  const uint64_t *w = reinterpret_cast<const uint64_t *>(T) + (p >> 3);
  const unsigned sh = unsigned(p & 7) * 8;
  const uint64_t a = w[0], b = w[1];
  return sh ? (a >> sh) | (b << (64 - sh)) : a;
}
__device__ inline void load16(const uint8_t *T, uint64_t p, uint64_t &lo, uint64_t &hi) {
  const uint64_t *w = reinterpret_cast<const uint64_t *>(T) + (p >> 3);
  const unsigned sh = unsigned(p & 7) * 8;
  const uint64_t a = w[0], b = w[1], c = w[2];
  lo = sh ? (a >> sh) | (b << (64 - sh)) : a;
  hi = sh ? (b >> sh) | (c << (64 - sh)) : b;
}
__device__ inline uint64_t low_bytes(unsigned n) {   // n in 0..7
  return (1ull << (8 * n)) - 1;
}

// the claimed exact LCP of rank r (< N): the byte, or the overflow table's
// value for r (lower bound by bisection; false: r is not in the table)
__device__ inline bool lcp_claim(const VCtx &c, uint64_t r, uint32_t l8, uint64_t &l) {
  if (l8 < 255) {
    l = l8;
    return true;
  }
  uint64_t lo = 0, hi = c.n_ovf;
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (c.ovf[2 * mid] < r) lo = mid + 1;
    else hi = mid;
  }
  if (lo >= c.n_ovf || c.ovf[2 * lo] != r) return false;
  l = c.ovf[2 * lo + 1];
  return true;
}

// T[x .. x + l) against T[y .. y + l) in one thread, 8 bytes a step; l < N - x
// and l < N - y.  Returns the bytes compared: l, or up to and including the
// first difference (eq = false)
__device__ inline uint64_t compare_thread(const uint8_t *T, uint64_t x, uint64_t y, uint64_t l,
                                          bool &eq) {
  for (uint64_t o = 0; o < l; o += 8) {
    uint64_t d = load8(T, x + o) ^ load8(T, y + o);
    if (l - o < 8) d &= low_bytes(unsigned(l - o));
    if (d) {
      eq = false;
      return o + (uint64_t(__ffsll((long long)d) - 1) >> 3) + 1;
    }
  }
  eq = true;
  return l;
}

// ---- perm + order + lcp, one pass over the ranks ---------------------------
// A wave takes 64 consecutive ranks, one per lane, so SA and L8 stream in
// whole lines.  Lane k's y = SA[i] is lane k + 1's x = SA[i - 1]: x, T[x],
// T[x - 1] and ISA[x + 1] come from the neighbour lane, not from memory (lane
// 0 loads them).  The random lines per rank are then T[y - 1 .. y],
// ISA[y - 1 .. y + 1], T[x + l], T[y + l] and, for a reducible rank, L8[j]
// and SA[j - 1].
template <class IdxT>
__global__ __launch_bounds__(256) void k_ranks(VCtx c, IdxArr<IdxT> SA, IdxArr<IdxT> ISA) {
  const uint64_t N = c.N;
  const uint8_t *T = c.T;
  const unsigned lane = threadIdx.x & 63;
  const uint64_t wave = (uint64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const uint64_t nwaves = (uint64_t(gridDim.x) * blockDim.x) >> 6;
  const bool do_sa = c.flags & SMASH_VERIFY_SA, do_lcp = c.flags & SMASH_VERIFY_LCP;
  unsigned long long perm_bad = 0, perm_first = kNone, order_bad = 0, order_first = kNone;
  unsigned long long lcp_bad = 0, lcp_first = kNone, n255 = 0, irr = 0, bytes = 0, longest = 0;
  for (uint64_t base = wave * 64; base < N; base += nwaves * 64) {
    const uint64_t i = base + lane;
    const bool act = i < N;
    unsigned long long y = N, iym = kNone, iy = kNone, iy1 = kNone;
    uint32_t l8 = 0, ty = 0, tym = 0;
    if (act) {
      y = SA[i];
      l8 = c.L8[i];
    }
    const bool yok = y < N;
    if (yok) {
      ty = T[y];
      iy = ISA[y];
      if (y > 0) {
        tym = T[y - 1];
        iym = ISA[y - 1];
      }
      if (y + 1 < N) iy1 = ISA[y + 1];
    }
    // the previous rank's suffix, from the lane below (every lane shuffles)
    unsigned long long x = __shfl_up(y, 1), ix1 = __shfl_up(iy1, 1);
    uint32_t tx = __shfl_up(ty, 1), txm = __shfl_up(tym, 1);
    if (lane == 0 && act && i > 0) {
      x = SA[i - 1];
      tx = txm = 0;
      ix1 = kNone;
      if (x < N) {
        tx = T[x];
        if (x > 0) txm = T[x - 1];
        if (x + 1 < N) ix1 = ISA[x + 1];
      }
    }
    if (!act) continue;   // (the wave's last trip: no shuffle follows)
    const bool xok = i > 0 && x < N;
    if (do_sa) {
      if (!yok || iy != i) {
        ++perm_bad;
        perm_first = i < perm_first ? i : perm_first;
      }
      bool good;
      if (i == 0) {
        good = y == N - 1 && ty == '$';
      } else {
        good = xok && yok &&
               (tx < ty || (tx == ty && x + 1 < N && y + 1 < N && ix1 < iy1));
      }
      if (!good) {
        ++order_bad;
        order_first = i < order_first ? i : order_first;
      }
    }
    if (!do_lcp) continue;
    n255 += l8 == 255;
    uint64_t l = 0;
    const bool have = lcp_claim(c, i, l8, l);
    bool good = false;
    if (i == 0) {
      good = have && l == 0;
    } else if (xok && yok && have && l < N - x && l < N - y && T[x + l] != T[y + l]) {
      if (x > 0 && y > 0 && txm == tym) {
        // reducible: the suffixes one position to the left are adjacent too
        const uint64_t j = iym;
        if (j >= 1 && j < N && SA[j - 1] == x - 1) {
          uint64_t lj = 0;
          good = lcp_claim(c, j, c.L8[j], lj) && lj == l + 1;
        }
      } else {
        ++irr;
        bool mine = l <= kThreadMax;
        if (!mine) {
          const unsigned long long slot = atomicAdd(&c.cnt[kWork], 1ull);
          if (slot < c.work_cap) c.work[slot] = WorkItem{i, x, y, l};
          else mine = true;   // a full list: the thread compares it itself
        }
        if (mine) {
          const uint64_t n = compare_thread(T, x, y, l, good);
          bytes += n;
          longest = n > longest ? n : longest;
        } else {
          good = true;        // k_long decides
        }
      }
    }
    if (!good) {
      ++lcp_bad;
      lcp_first = i < lcp_first ? i : lcp_first;
    }
  }
  if (do_sa) {
    flush_sum(&c.cnt[kPermBad], perm_bad);
    flush_min(&c.cnt[kPermFirst], perm_first);
    flush_sum(&c.cnt[kOrderBad], order_bad);
    flush_min(&c.cnt[kOrderFirst], order_first);
  }
  if (do_lcp) {
    flush_sum(&c.cnt[kLcpBad], lcp_bad);
    flush_min(&c.cnt[kLcpFirst], lcp_first);
    flush_sum(&c.cnt[kN255], n255);
    flush_sum(&c.cnt[kIrr], irr);
    flush_sum(&c.cnt[kBytes], bytes);
    flush_max(&c.cnt[kLongest], longest);
  }
}

// The work list: one wave per entry, 16 bytes a lane a step (1 KiB of each
// side per step), any pair of alignments (load16), out at the first step that
// holds a difference.  Every entry has l < N - x and l < N - y (k_ranks).
__global__ __launch_bounds__(256) void k_long(VCtx c) {
  const uint8_t *T = c.T;
  const unsigned lane = threadIdx.x & 63;
  const uint64_t wave = (uint64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const uint64_t nwaves = (uint64_t(gridDim.x) * blockDim.x) >> 6;
  const uint64_t n = c.cnt[kWork] < c.work_cap ? c.cnt[kWork] : c.work_cap;
  unsigned long long bad = 0, first = kNone, bytes = 0, longest = 0;
  for (uint64_t e = wave; e < n; e += nwaves) {
    const WorkItem w = c.work[e];
    unsigned long long stop = kNone;   // offset of the first difference
    for (uint64_t o0 = 0; o0 < w.l; o0 += 1024) {
      const uint64_t o = o0 + 16 * lane;
      unsigned long long at = kNone;
      if (o < w.l) {
        uint64_t a0, a1, b0, b1;
        load16(T, w.x + o, a0, a1);
        load16(T, w.y + o, b0, b1);
        uint64_t d0 = a0 ^ b0, d1 = a1 ^ b1;
        const uint64_t left = w.l - o;
        if (left < 8) {
          d0 &= low_bytes(unsigned(left));
          d1 = 0;
        } else if (left < 16) {
          d1 &= low_bytes(unsigned(left - 8));
        }
        if (d0) at = o + (uint64_t(__ffsll((long long)d0) - 1) >> 3);
        else if (d1) at = o + 8 + (uint64_t(__ffsll((long long)d1) - 1) >> 3);
      }
      const unsigned long long hit = __ballot(at != kNone);
      if (hit) {   // the lowest lane holds the lowest offset
        stop = __shfl(at, __ffsll((long long)hit) - 1);
        break;
      }
    }
    if (lane == 0) {
      const uint64_t cmp = stop == kNone ? w.l : stop + 1;
      bytes += cmp;
      longest = cmp > longest ? cmp : longest;
      if (stop != kNone) {
        ++bad;
        first = w.rank < first ? w.rank : first;
      }
    }
  }
  flush_sum(&c.cnt[kLcpBad], bad);
  flush_min(&c.cnt[kLcpFirst], first);
  flush_sum(&c.cnt[kBytes], bytes);
  flush_max(&c.cnt[kLongest], longest);
}

// the overflow table: {idx, val} with idx < N ascending, L8[idx] == 255, val >= 255
__global__ __launch_bounds__(256) void k_ovf(VCtx c) {
  unsigned long long bad = 0, first = kNone;
  const uint64_t stride = uint64_t(gridDim.x) * blockDim.x;
  for (uint64_t e = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; e < c.n_ovf; e += stride) {
    const uint64_t idx = c.ovf[2 * e], val = c.ovf[2 * e + 1];
    const bool b = idx >= c.N || c.L8[idx] != 255 || val < 255 ||
                   (e > 0 && c.ovf[2 * (e - 1)] >= idx);
    if (b) {
      ++bad;
      first = e < first ? e : first;
    }
  }
  flush_sum(&c.cnt[kOvfBad], bad);
  flush_min(&c.cnt[kOvfFirst], first);
}

// ---- layout ------------------------------------------------------------------
// separators in the text (16 bytes a thread; the zero pad past N holds none)
__global__ __launch_bounds__(256) void k_seps(VCtx c) {
  unsigned long long ticks = 0, dollars = 0;
  const uint64_t n16 = (c.N + 15) >> 4, stride = uint64_t(gridDim.x) * blockDim.x;
  const uint4 *p = reinterpret_cast<const uint4 *>(c.T);
  for (uint64_t q = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; q < n16; q += stride) {
    const uint4 v = p[q];
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const uint32_t ch = (w[k] >> (8 * b)) & 0xFF;
        ticks += ch == '`';
        dollars += ch == '$';
      }
  }
  flush_sum(&c.cnt[kTicks], ticks);
  flush_sum(&c.cnt[kDollars], dollars);
}

// the contig table against the text: entry q ends inside the text at its
// separator ('$' at N - 1 for the last), the next entry starts right after
// it, and with rcref the two entries of a contig have one size
__global__ void k_table(VCtx c, const uint64_t *startpos, const uint64_t *sizes, uint32_t n_seq,
                        int rcref) {
  unsigned long long bad = 0, first = kNone;
  const uint64_t N = c.N;
  for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < n_seq;
       q += gridDim.x * blockDim.x) {
    const uint64_t sp = startpos[q], sz = sizes[q];
    const bool inr = sp <= N - 1 && sz <= N - 1 - sp;
    const uint64_t end = inr ? sp + sz : N - 1;
    const bool last = q == n_seq - 1;
    bool b = !inr;
    if (inr) {
      if (last) b = end != N - 1 || c.T[end] != '$';
      else b = c.T[end] != '`' || startpos[q + 1] != end + 1;
    }
    if (rcref && sizes[q ^ 1u] != sz) b = true;   // (n_seq is even with rcref)
    if (b) {
      ++bad;
      first = end < first ? end : first;
    }
  }
  flush_sum(&c.cnt[kLayoutBad], bad);
  flush_min(&c.cnt[kLayoutFirst], first);
}

// rc halves of the contigs whose two entries are in range and of one size:
// work item w of pair k (cum[k] <= w < cum[k + 1]) is base t = w - cum[k]
struct RcPair {
  uint64_t sp0, sp1, size, cum;
};
__global__ __launch_bounds__(256) void k_rc(VCtx c, const RcPair *pairs, uint32_t n_pairs,
                                            uint64_t total) {
  unsigned long long bad = 0, first = kNone;
  const uint64_t stride = uint64_t(gridDim.x) * blockDim.x;
  for (uint64_t w = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; w < total; w += stride) {
    uint32_t lo = 0, hi = n_pairs;   // the last pair with cum <= w
    while (hi - lo > 1) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (pairs[mid].cum <= w) lo = mid;
      else hi = mid;
    }
    const RcPair p = pairs[lo];
    const uint64_t t = w - p.cum;
    if (t >= p.size) continue;   // (cannot happen: cum is the prefix sum of size)
    if (c.T[p.sp1 + t] != comp_base(c.T[p.sp0 + p.size - 1 - t])) {
      ++bad;
      first = p.sp1 + t < first ? p.sp1 + t : first;
    }
  }
  flush_sum(&c.cnt[kLayoutBad], bad);
  flush_min(&c.cnt[kLayoutFirst], first);
}

// ---- map ---------------------------------------------------------------------
// n bases: the recomputed [left, right] pairs against the map's (both 2-byte
// aligned); off0 = the map.bin offset of ref[0]
__global__ __launch_bounds__(256) void k_mapcmp(const uint16_t *ref, const uint16_t *map,
                                                uint64_t n, uint64_t off0,
                                                unsigned long long *cnt) {
  unsigned long long bad = 0, first = kNone;
  const uint64_t stride = uint64_t(gridDim.x) * blockDim.x;
  for (uint64_t g = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; g < n; g += stride) {
    const uint32_t d = uint32_t(ref[g]) ^ uint32_t(map[g]);
    if (d) {
      bad += ((d & 0xFF) != 0) + ((d >> 8) != 0);
      const uint64_t at = off0 + 2 * g + ((d & 0xFF) ? 0 : 1);
      first = at < first ? at : first;
    }
  }
  flush_sum(&cnt[kMapBad], bad);
  flush_min(&cnt[kMapFirst], first);
}

double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch())
      .count();
}

struct DevBuf {   // freed on every way out
  void *p = nullptr;
  ~DevBuf() { dfree(p); }
};

template <class IdxT>
void launch_ranks(const VCtx &c, const smash_index *ix, unsigned grid, hipStream_t s) {
  IdxArr<IdxT> SA{static_cast<const IdxT *>(ix->d_sa), ix->pos_mask};
  IdxArr<IdxT> ISA{static_cast<const IdxT *>(ix->d_isa), ix->pos_mask};
  k_ranks<IdxT><<<grid, 256, 0, s>>>(c, SA, ISA);
}

}  // namespace

int verify_impl(const smash_index *ix, uint32_t flags, smash_verify_report *out, hipStream_t s,
                bool proven) {
  const double t0 = now_s();
  memset(out, 0, sizeof(*out));
  out->layout_first = out->perm_first = out->order_first = out->lcp_first = out->ovf_first =
      out->map_first = kNone;
  const uint64_t N = ix->N;
  if (N < 2 || ix->n_seq == 0) {   // (a header of a loaded cache: N - 1 is used below)
    set_error("smash_index_verify: a text of fewer than 2 bytes or an empty contig table");
    return SMASH_ERR_ARG;
  }
  try {
    SMASH_HIPX(hipSetDevice(ix->device));
    int cus = 0;
    SMASH_HIPX(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ix->device));
    const unsigned cap = unsigned(cus > 0 ? cus : 64) * 8;   // blocks: the rest is grid-stride
    DevBuf cnt_b, work_b;
    cnt_b.p = dalloc<unsigned long long>(kCounters);
    unsigned long long h[kCounters];
    for (int k = 0; k < kCounters; ++k) h[k] = 0;
    h[kLayoutFirst] = h[kPermFirst] = h[kOrderFirst] = h[kLcpFirst] = h[kOvfFirst] =
        h[kMapFirst] = kNone;
    SMASH_HIPX(hipMemcpyAsync(cnt_b.p, h, sizeof(h), hipMemcpyHostToDevice, s));
    SMASH_HIPX(hipStreamSynchronize(s));   // (h is reused below)
    VCtx c;
    c.T = ix->d_text;
    c.L8 = ix->d_lcp8;
    c.ovf = ix->d_ovf;
    c.n_ovf = ix->n_ovf;
    c.N = N;
    c.cnt = static_cast<unsigned long long *>(cnt_b.p);
    c.work = nullptr;
    c.work_cap = 0;
    c.flags = flags;
    const char *tv = getenv("SMASH_VERIFY_TIMES");   // per-stage seconds on stderr
    const bool times = tv && *tv == '1';
    double t_prev = now_s();
    auto stage = [&](const char *what) {
      if (!times) return;
      SMASH_HIPX(hipStreamSynchronize(s));
      const double t = now_s();
      fprintf(stderr, "smash_index_verify: %-8s %.6f s\n", what, t - t_prev);
      t_prev = t;
    };

    if (flags & SMASH_VERIFY_LAYOUT) {
      k_seps<<<grid_for((N + 15) >> 4, 256, cap), 256, 0, s>>>(c);
      SMASH_HIPX(hipGetLastError());
      k_table<<<grid_for(ix->n_seq, 64, cap), 64, 0, s>>>(c, ix->d_startpos, ix->d_sizes,
                                                          ix->n_seq, ix->rcref ? 1 : 0);
      SMASH_HIPX(hipGetLastError());
      DevBuf pairs_b;
      if (ix->rcref) {
        std::vector<RcPair> pairs;
        uint64_t total = 0;
        for (uint32_t q = 0; q + 1 < ix->n_seq; q += 2) {
          const uint64_t sp0 = ix->startpos[q], sz = ix->sizes[q], sp1 = ix->startpos[q + 1];
          const bool in0 = sp0 <= N - 1 && sz <= N - 1 - sp0;
          const bool in1 = sp1 <= N - 1 && sz <= N - 1 - sp1;
          if (!in0 || !in1 || ix->sizes[q + 1] != sz || sz == 0) continue;
          pairs.push_back(RcPair{sp0, sp1, sz, total});
          total += sz;
        }
        if (total) {
          pairs_b.p = dalloc<RcPair>(pairs.size());
          SMASH_HIPX(hipMemcpyAsync(pairs_b.p, pairs.data(), sizeof(RcPair) * pairs.size(),
                                    hipMemcpyHostToDevice, s));
          k_rc<<<grid_for(total, 256, cap), 256, 0, s>>>(c, static_cast<const RcPair *>(pairs_b.p),
                                                         uint32_t(pairs.size()), total);
          SMASH_HIPX(hipGetLastError());
          SMASH_HIPX(hipStreamSynchronize(s));   // (pairs is a host local)
        }
      }
      out->checked |= SMASH_VERIFY_LAYOUT;
      stage("layout");
    }

    if (flags & (SMASH_VERIFY_SA | SMASH_VERIFY_LCP)) {
      if (flags & SMASH_VERIFY_LCP) {
        c.work_cap = std::min<uint64_t>(kWorkCap, N / 16 + 1024);
        work_b.p = dalloc<WorkItem>(c.work_cap);
        c.work = static_cast<WorkItem *>(work_b.p);
      }
      const unsigned grid = grid_for(N, 256, cap);
      if (ix->idx_bytes == 4) launch_ranks<uint32_t>(c, ix, grid, s);
      else launch_ranks<uint64_t>(c, ix, grid, s);
      SMASH_HIPX(hipGetLastError());
      stage("ranks");
      if (flags & SMASH_VERIFY_LCP) {
        unsigned long long n_work = 0;
        SMASH_HIPX(hipMemcpyAsync(&n_work, c.cnt + kWork, 8, hipMemcpyDeviceToHost, s));
        SMASH_HIPX(hipStreamSynchronize(s));
        n_work = std::min<unsigned long long>(n_work, c.work_cap);
        if (n_work) {
          k_long<<<grid_for(n_work, 4, cap), 256, 0, s>>>(c);
          SMASH_HIPX(hipGetLastError());
        }
        stage("long");
        if (ix->n_ovf) {
          k_ovf<<<grid_for(ix->n_ovf, 256, cap), 256, 0, s>>>(c);
          SMASH_HIPX(hipGetLastError());
        }
        stage("ovf");
      }
      out->checked |= flags & (SMASH_VERIFY_SA | SMASH_VERIFY_LCP);
    }

    SMASH_HIPX(hipMemcpyAsync(h, cnt_b.p, sizeof(h), hipMemcpyDeviceToHost, s));
    SMASH_HIPX(hipStreamSynchronize(s));
    if (flags & SMASH_VERIFY_LAYOUT) {
      const uint64_t want = ix->n_seq - 1;
      const uint64_t extra = (h[kTicks] > want ? h[kTicks] - want : want - h[kTicks]) +
                             (h[kDollars] > 1 ? h[kDollars] - 1 : 1 - h[kDollars]);
      h[kLayoutBad] += extra;
      // a separator count has no position of its own: the end of the text
      if (extra && h[kLayoutFirst] == kNone) h[kLayoutFirst] = N - 1;
    }
    const bool lcp_ran = out->checked & SMASH_VERIFY_LCP;
    bool clean = !h[kLayoutBad] && !h[kPermBad] && !h[kOrderBad] && !h[kLcpBad] && !h[kOvfBad] &&
                 (!lcp_ran || h[kN255] == ix->n_ovf);

    // the map: the scan trusts the arrays, so only behind a clean proof
    const uint32_t proof = SMASH_VERIFY_LAYOUT | SMASH_VERIFY_SA | SMASH_VERIFY_LCP;
    if ((flags & SMASH_VERIFY_MAP) && ix->d_map && ix->rcref && ix->d_uniq &&
        (proven || ((out->checked & proof) == proof && clean))) {
      uint64_t total = 0;
      for (uint32_t q = 0; q < ix->n_seq; q += 2) total += ix->sizes[q];
      if (ix->map_bytes != 2 + 2 * total) {
        h[kMapBad] = 1;   // (a map of another genome's size: nothing to compare)
        h[kMapFirst] = 0;
      } else if (total) {
        DevBuf scratch;
        scratch.p = dalloc<uint8_t>(2 * std::min(total, kMapWindow));
        for (uint64_t b = 0; b < total; b += kMapWindow) {
          const uint64_t e = std::min(total, b + kMapWindow);
          if (smash_mappability_scan(ix, b, e, 36, static_cast<uint8_t *>(scratch.p), nullptr,
                                     nullptr, 0, nullptr, nullptr, s) != SMASH_OK)
            throw hip_failure{std::string("smash_index_verify: ") + smash_last_error()};
          k_mapcmp<<<grid_for(e - b, 256, cap), 256, 0, s>>>(
              static_cast<const uint16_t *>(scratch.p),
              reinterpret_cast<const uint16_t *>(ix->d_map + 2 + 2 * b), e - b, 2 + 2 * b, c.cnt);
          SMASH_HIPX(hipGetLastError());
        }
        unsigned long long m[2];
        SMASH_HIPX(hipMemcpyAsync(m, c.cnt + kMapBad, 16, hipMemcpyDeviceToHost, s));
        SMASH_HIPX(hipStreamSynchronize(s));
        h[kMapBad] = m[0];
        h[kMapFirst] = m[1];
      }
      out->checked |= SMASH_VERIFY_MAP;
      clean = clean && !h[kMapBad];
      stage("map");
    }
    out->layout_bad = h[kLayoutBad]; out->layout_first = h[kLayoutFirst];
    out->perm_bad = h[kPermBad];     out->perm_first = h[kPermFirst];
    out->order_bad = h[kOrderBad];   out->order_first = h[kOrderFirst];
    out->lcp_bad = h[kLcpBad];       out->lcp_first = h[kLcpFirst];
    out->ovf_bad = h[kOvfBad];       out->ovf_first = h[kOvfFirst];
    out->map_bad = h[kMapBad];       out->map_first = h[kMapFirst];
    out->n_lcp255 = h[kN255];
    out->lcp_irreducible = h[kIrr];
    out->lcp_bytes_compared = h[kBytes];
    out->lcp_longest = h[kLongest];
    out->ok = clean ? 1 : 0;
  } catch (hip_failure &f) {
    set_error(f.what);
    return f.what.find("hipMalloc") != std::string::npos ? SMASH_ERR_NOMEM : SMASH_ERR_HIP;
  }
  out->seconds = now_s() - t0;
  return SMASH_OK;
}

std::string verify_finding(const smash_verify_report &r, uint64_t n_ovf) {
  auto say = [](const char *what, uint64_t bad, const char *unit, uint64_t first) {
    return std::string(what) + ": " + std::to_string(bad) + " bad, first at " + unit + " " +
           std::to_string(first);
  };
  if (r.layout_bad) return say("layout", r.layout_bad, "text position", r.layout_first);
  if (r.perm_bad) return say("perm (ISA[SA[i]] == i)", r.perm_bad, "rank", r.perm_first);
  if (r.order_bad) return say("order (suffix order)", r.order_bad, "rank", r.order_first);
  if (r.ovf_bad) return say("ovf (LCP overflow table)", r.ovf_bad, "entry", r.ovf_first);
  if ((r.checked & SMASH_VERIFY_LCP) && r.n_lcp255 != n_ovf)
    return "ovf (LCP overflow table): " + std::to_string(r.n_lcp255) + " ranks with LCP byte 255, " +
           std::to_string(n_ovf) + " table entries" +
           (r.lcp_bad ? ", first unproven LCP at rank " + std::to_string(r.lcp_first) : "");
  if (r.lcp_bad) return say("lcp (exact LCP)", r.lcp_bad, "rank", r.lcp_first);
  if (r.map_bad) return say("map (map.bin)", r.map_bad, "map.bin byte", r.map_first);
  return "";
}

}  // namespace smash

using namespace smash;

extern "C" int smash_index_verify(const smash_index *ix, uint32_t flags, smash_verify_report *out,
                                  void *stream) {
  if (!ix || !out || !flags || (flags & ~SMASH_VERIFY_ALL)) {
    set_error("smash_index_verify: bad arguments");
    return SMASH_ERR_ARG;
  }
  return verify_impl(ix, flags, out, static_cast<hipStream_t>(stream), false);
}
