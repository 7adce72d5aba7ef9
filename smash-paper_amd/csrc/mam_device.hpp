// smash-paper_amd/csrc/mam_device.hpp -- device-side MAM search (one lane).
//
// Semantics of longSA::MAM (longSA.cpp:503-536), traverse (:297-316),
// top_down_faster (:322-380), expand_link (longSA.h:158-174) and
// is_leftmaximal (:540-546); characters compare as signed chars widened to
// int64 like the reference.
#pragma once
#include "common.hpp"

namespace smash {

template <class IdxT>
struct DevIndex {
  const uint8_t *T;     // text (+64 zero bytes)
  IdxArr<IdxT> SA;      // positions only (the packed hints masked off)
  IdxArr<IdxT> ISA;
  const uint8_t *L8;    // min(LCP,255)
  const uint8_t *U;     // per-position unique-length bytes (aux_build.hip)
  const uint64_t *KT;   // k-mer -> {lo, hi} + (k+2)-mer presence bits (common.hpp)
  uint64_t N, logN;
  int K, B;
  uint64_t in_text[4];  // bytes that occur in the text
};

template <class IdxT>
inline DevIndex<IdxT> make_dev_index(const smash_index *ix) {
  DevIndex<IdxT> x;
  x.T = ix->d_text;
  x.SA = IdxArr<IdxT>{static_cast<const IdxT *>(ix->d_sa), ix->pos_mask};
  x.ISA = IdxArr<IdxT>{static_cast<const IdxT *>(ix->d_isa), ix->pos_mask};
  x.L8 = ix->d_lcp8;
  x.U = ix->d_uniq;
  x.KT = ix->d_kmer;
  x.N = ix->N;
  x.logN = ix->logN;
  x.K = int(ix->kmer_k);
  x.B = int(ix->bitmap_b);
  for (int k = 0; k < 4; ++k) x.in_text[k] = ix->in_text[k];
  return x;
}

struct MatchSink {
  uint64_t *out;
  uint32_t cap, n;
  __device__ void emit(uint64_t ref, uint64_t q, uint64_t len) {
    if (n < cap) out[n] = pack_match(ref, uint32_t(q), uint32_t(len));
    ++n;
  }
};

__device__ __forceinline__ int64_t sch(uint8_t c) { return int64_t(int8_t(c)); }

// top_down_faster: narrow [start,end] at depth i by character c.
template <class IdxT>
__device__ __forceinline__ bool td_faster(const DevIndex<IdxT> &x, int64_t c,
                                          uint64_t i, uint64_t &start,
                                          uint64_t &end) {
  uint64_t l, r, m, r2 = end, l2 = start;
  int64_t v;
  bool found = false;
  const int64_t cf = c - sch(x.T[uint64_t(x.SA[start]) + i]);
  const int64_t cl = c - sch(x.T[uint64_t(x.SA[end]) + i]);
  if (cf < 0) {
    l = start + 1;
    l2 = start;
  } else if (cl > 0) {
    l = end + 1;
    l2 = end;
  } else {
    l = start;
    r = end;
    if (cf == 0) {
      found = true;
      r2 = r;
    } else {
      while (r > l + 1) {
        m = (l + r) >> 1;
        v = c - sch(x.T[uint64_t(x.SA[m]) + i]);
        if (v <= 0) {
          if (!found && v == 0) {
            found = true;
            l2 = m;
            r2 = r;
          }
          r = m;
        } else {
          l = m;
        }
      }
      l = r;
    }
    if (!found) l2 = l - 1;
    if (cl == 0) {
      l2 = end;
    } else {
      while (r2 > l2 + 1) {
        m = (l2 + r2) >> 1;
        v = c - sch(x.T[uint64_t(x.SA[m]) + i]);
        if (v < 0) r2 = m;
        else l2 = m;
      }
    }
  }
  start = l;
  end = l2;
  return l <= l2;
}

template <class IdxT>
__device__ __forceinline__ bool expand_link(const DevIndex<IdxT> &x,
                                            uint64_t depth, uint64_t &start,
                                            uint64_t &end) {
  const uint64_t thresh = 2 * depth * x.logN;
  uint64_t exp = 0, s = start, e = end;
  while (uint64_t(x.L8[s]) >= depth) {
    if (++exp >= thresh) return false;
    --s;
  }
  while (e < x.N - 1 && uint64_t(x.L8[e + 1]) >= depth) {
    if (++exp >= thresh) return false;
    ++e;
  }
  start = s;
  end = e;
  return true;
}

// P: this lane's read (LDS), length L.  The reference's probe sequence,
// statement by statement (SMASH_MODE_MAM_PLAIN).
template <class IdxT>
__device__ void mam_read_plain(const DevIndex<IdxT> &x, const uint8_t *P, uint32_t L,
                               uint32_t min_len, MatchSink &sink) {
  const uint64_t N = x.N;
  uint64_t depth = 0, start = 0, end = N - 1;
  uint64_t prefix = 0;
  while (prefix < L) {
    // traverse(P, prefix, cur, P.length())
    if (depth < L) {
      while (prefix + depth < L) {
        uint64_t s = start, e = end;
        if (!td_faster(x, sch(P[prefix + depth]), depth, s, e)) break;
        depth += 1;
        start = s;
        end = e;
        if (depth == L) break;
      }
    }
    if (depth <= 1) {
      depth = 0;
      start = 0;
      end = N - 1;
      ++prefix;
      continue;
    }
    if (end == start && depth >= min_len) {
      const uint64_t p2 = x.SA[start];
      const bool lm = (prefix == 0 || p2 == 0) ? true
                      : (sch(P[prefix - 1]) != sch(x.T[p2 - 1]));
      if (lm) sink.emit(p2, prefix, depth);
    }
    do {
      depth = depth - 1;
      start = x.ISA[uint64_t(x.SA[start]) + 1];
      end = x.ISA[uint64_t(x.SA[end]) + 1];
      ++prefix;
      if (depth == 0 || !expand_link(x, depth, start, end)) {
        depth = 0;
        start = 0;
        end = N - 1;
        break;
      }
    } while (depth > 0 && end == start);
  }
}

// ---------------------------------------------------------------------------
// Word-level helpers of the accelerated searches (SMASH_MODE_MAM: k_mam_sm,
// mam_sm.hpp; MEM: mem.hip).  The accelerated MAM algorithm itself is stated
// straight-line on the CPU: orc_mam_v3, oracle/smash_oracle.c.
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint64_t load8(const uint8_t *T, uint64_t a) {
  const uint64_t *w = reinterpret_cast<const uint64_t *>(T);
  const uint64_t q = a >> 3, sh = (a & 7) * 8;
  const uint64_t lo = w[q];
  if (sh == 0) return lo;
  return (lo >> sh) | (w[q + 1] << (64 - sh));
}

__device__ __forceinline__ int acgt_code(uint8_t c) {
  return c == 'a' ? 0 : c == 'c' ? 1 : c == 'g' ? 2 : c == 't' ? 3 : -1;
}

// 8 read bytes at byte offset `off` of an LDS row (row 4-byte aligned and
// padded; bytes past the read are masked by the callers)
// (v_alignbyte_b32: the low dword of {hi, lo} >> 8 * (s & 3); the host
// emulation substitutes its own)
#ifndef SM_ALIGNBYTE
#define SM_ALIGNBYTE(hi, lo, s) __builtin_amdgcn_alignbyte(hi, lo, s)
#endif
__device__ __forceinline__ uint64_t lds_load8(const uint8_t *P, uint64_t off) {
  // three aligned words, two byte-aligns (no 64-bit shifts, no select on the
  // offset): the rows carry the third word's over-read
  const uint32_t *w = reinterpret_cast<const uint32_t *>(P);
  const uint32_t q = uint32_t(off) >> 2, s = uint32_t(off) & 3;
  const uint32_t w0 = w[q], w1 = w[q + 1], w2 = w[q + 2];
  return uint64_t(SM_ALIGNBYTE(w1, w0, s)) | (uint64_t(SM_ALIGNBYTE(w2, w1, s)) << 32);
}

// bytes of agreement of two 8-byte words, capped at lim (<= 8)
// (ctz with 64 for zero: v_ffbl pairs with no compare-and-select on the
// 64-bit difference; the host emulation substitutes its own)
#ifndef SM_CTZ64
#define SM_CTZ64(x) __builtin_ctzg(x, 64)
#endif
__device__ __forceinline__ uint32_t agree8(uint64_t a, uint64_t b, uint32_t lim) {
  const uint32_t k = uint32_t(SM_CTZ64(a ^ b)) >> 3;
  return k < lim ? k : lim;
}

}  // namespace smash
