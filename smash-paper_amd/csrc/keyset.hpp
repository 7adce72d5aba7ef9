// smash-paper_amd/csrc/keyset.hpp -- the persistent pair-key set: everything
// that knows the table slot / ref / arena record format, the claim / decide
// protocol over it (once, for the single-GPU pairs and for an owner's
// received keys) and the set's growth.  Included by pipeline.hip only, below
// its per-pair helpers (HitRows, mix64, wave_stats, the export header).
#pragma once

namespace smash {
namespace {

// The persistent pair-key set of smashMEM.py:149,217-228 (dupeSet), exact:
// a key is the pair's kept hit list (tid << 48 | pos0 per hit, r1 then r2 in
// HI order, smashMEM.py:122-131).  Open addressing on the 64-bit hash `hi`;
// slot = {hi, ref} (ref 0: the inserting thread has not stored it yet).  A
// key's record is kept in one of two places, and its ref says which:
//   * a row ref, g + 1 (bits 39.. clear): the key has at most kHitHead words
//     and came from pair g of the single-GPU run (pairs counted from the last
//     reset).  The record is that pair's head row (HitRows, d_hhead) and its
//     word count (d_nk): both hold every pair of the run, so nothing is
//     copied.  A smaller g is an earlier pair, in or before the batch, so the
//     claim's atomicMin alone leaves the slot naming the key's first pair.
//   * an arena ref, epoch << 40 | kRefPub | (1 + arena offset of the record
//     [lo, nk, words]): a single-GPU key of more than kHitHead words (its
//     full row lasts one batch), or a key an owner received (transient
//     buffers).  Until its decide publishes it, such a key's slot holds its
//     claim: g + 1 (single GPU) or epoch << 40 | (j + 1) (owner).
// A hash match counts as the same key only when the word count and every hit
// word agree (and, against an arena record, the second hash lo), so a hash
// collision is a different key (it goes on probing), never a false duplicate.
//
// Slot accesses are relaxed, with no per-key release / acquire (agent-scope
// fences write back / invalidate the XCD's L2 on gfx950 and made the round-2
// insert kernel 5 ms per 2 M pairs): a launch compares only against records
// of earlier launches (rows and arena records), which are visible across the
// kernel boundary, and against this launch's claims through the claimers' own
// input rows (the claim / decide kernels below).  Epochs run from 1 and wrap
// after 2^24 launches; a row ref's epoch field is 0.
//
// With a sample table set (smash_pipeline_samples) a key is the hit list AND
// the sample of its pair: the sample-aware claim / decide (SamplePairKeys)
// salt the hash hi the table sees with the sample, so equal hit lists of two
// samples start two probe chains, and compare the sample exactly wherever
// they compare the words: a row record's is that of its pair g (a bisect
// over the table, SampleTab::of), an arena record keeps sample + 1 in the high
// half of its nk word (0 there: a record of a run without a table).  An owner
// of a run with a sharded table (smash_pipeline_samples_sharded) does the same
// over its received keys (RecvSampleKeys): the sample comes in the header's
// second word, every record is an arena record.
constexpr int kRefShift = 40;
// a published arena ref carries kRefPub; row refs and claims do not
constexpr uint64_t kRefPub = 1ull << 39;
// where the claims find the set's records
struct KeyStore {
  uint64_t *table;
  uint64_t mask;
  const uint64_t *arena;
  const uint64_t *rows;   // [row_cap][kHitHead]: the run's head rows (d_hhead)
  const int32_t *row_nk;  // [row_cap]: their word counts (d_nk)
};
struct KeyRef {
  const uint64_t *w;   // the key's hit words
  uint32_t nk;
  uint64_t lo;
};

__device__ bool same_key(const uint64_t *rec, const KeyRef &k) {
  if (rec[0] != k.lo || rec[1] != k.nk) return false;
  for (uint32_t i = 0; i < k.nk; ++i)
    if (rec[2 + i] != k.w[i]) return false;
  return true;
}

// against an arena record of a run with a sample table: the nk word's high
// half is the record's sample + 1
__device__ bool same_key(const uint64_t *rec, const KeyRef &k, uint32_t smp) {
  if (rec[0] != k.lo || rec[1] != (uint64_t(smp + 1) << 32 | k.nk)) return false;
  for (uint32_t i = 0; i < k.nk; ++i)
    if (rec[2 + i] != k.w[i]) return false;
  return true;
}

__device__ bool same_key(const KeyRef &a, const KeyRef &b) {
  if (a.lo != b.lo || a.nk != b.nk) return false;
  for (uint32_t i = 0; i < a.nk; ++i)
    if (a.w[i] != b.w[i]) return false;
  return true;
}

// against the row record of the run's pair g (row keys only: a longer key is
// never equal to one)
__device__ bool same_key(const KeyStore &st, uint64_t g, const KeyRef &k) {
  if (k.nk > kHitHead || st.row_nk[g] != int32_t(k.nk)) return false;
  const uint64_t *r = st.rows + g * kHitHead;
  for (uint32_t i = 0; i < k.nk; ++i)
    if (r[i] != k.w[i]) return false;
  return true;
}

// the pair key's two hashes from its hit words, exactly as k_post /
// k_post_fast fold them while they build the key (a word is tid << 48 | pos0,
// pos0 < 2^48, so the | there is the ^ here)
__device__ inline void key_hashes(const uint64_t *w, uint32_t nk, uint64_t mask, uint64_t &hh,
                                  uint64_t &hl) {
  hh = 0x9E3779B97F4A7C15ull;
  hl = 0xD1B54A32D192ED03ull;
  for (uint32_t i = 0; i < nk; ++i) {
    const uint64_t x = w[i];
    hh = mix64(hh ^ x) + 0x632BE59BD9B4E019ull;
    hl = mix64(hl + x * 0x9E3779B97F4A7C15ull) ^ (hl >> 29);
  }
  hh = (mix64(hh ^ uint64_t(nk)) & mask) | 1;
  hl = (mix64(hl + uint64_t(nk)) & mask) | 1;
}

// the first slot of a key's (linear) probe sequence
__host__ __device__ __forceinline__ uint64_t key_home(uint64_t hi, uint64_t mask) {
  return (hi ^ (hi >> 31)) & mask;
}

// the wave's inclusive prefix of v (every lane calls it) and its total
__device__ __forceinline__ uint32_t wave_incl(uint32_t v, uint32_t &total) {
  const uint32_t lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t y = __shfl_up(v, d, 64);
    if (lane >= uint32_t(d)) v += y;
  }
  total = __shfl(v, 63, 64);
  return v;
}

// The lane whose list holds word t of the wave's concatenated lists (lane
// order; incl = the inclusive prefix of the lists' sizes): the first lane l
// with incl(l) > t, lane 63 when t is past the end.  before: the words of the
// lanes below l, so t - before is the word's index in l's list.  Every lane
// of the wave calls it.
__device__ __forceinline__ uint32_t wave_word_owner(uint32_t incl, uint32_t t, uint32_t &before) {
  uint32_t l = 0;
#pragma unroll
  for (uint32_t step = 32; step; step >>= 1)
    if (uint32_t(__shfl(int(incl), int(l + step - 1), 64)) <= t) l += step;
  l = l < 63u ? l : 63u;
  // (the shuffle runs on every lane, outside the select: a cross-lane read
  // under a partial exec mask returns 0 from the lanes it excludes)
  const uint32_t prev = uint32_t(__shfl(int(incl), int((l + 63u) & 63u), 64));
  before = l ? prev : 0u;
  return l;
}

// the decide kernels take kDecGroups groups of 64 consecutive keys per wave
// per trip and reserve their arena space with ONE atomic: the arena top is a
// single address, and one atomic per 64 keys (~100 k per 6.25 M-pair batch)
// serialised on its L2 channel for ~1 ms
constexpr uint32_t kDecGroups = 4;

// The key records {hash lo, nk, hit words} of a wave's winners, written by
// the whole wave: the decide kernels give each group of 64 keys one
// contiguous arena range
// (lane l's record at off(l), incl = the inclusive prefix of the record
// sizes), so word t of the range belongs to the first lane l with
// incl(l) > t and consecutive lanes store consecutive words (a lane-per-record
// loop stores 64 words a record apart per instruction).  ok: the lane's
// record fits the arena; lo / m / src: its hash lo, word count and words.
// Every lane of the wave calls it (wave-uniform trip count).  SMP: the nk word
// carries smp + 1 in its high half (the key's sample).
template <bool SMP>
__device__ __forceinline__ void wave_fill_records(uint64_t *arena, uint64_t off, uint32_t incl,
                                                  uint32_t total, bool ok, uint64_t lo, uint32_t m,
                                                  const uint64_t *src, uint32_t smp) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t srcv = reinterpret_cast<uint64_t>(src);
  for (uint32_t t0 = 0; t0 < total; t0 += 64) {
    const uint32_t t = t0 + lane;
    uint32_t before;
    const uint32_t l = wave_word_owner(incl, t, before);
    const uint32_t r = t - before;   // word r of lane l's record
    const bool lok = __shfl(int(ok), int(l), 64) != 0;
    const uint64_t loff = __shfl(off, int(l), 64), llo = __shfl(lo, int(l), 64);
    const uint32_t lm = uint32_t(__shfl(int(m), int(l), 64));
    const uint64_t *ls = reinterpret_cast<const uint64_t *>(__shfl(srcv, int(l), 64));
    if constexpr (SMP) {
      const uint64_t nkw = uint64_t(uint32_t(__shfl(int(smp), int(l), 64)) + 1) << 32 | lm;
      if (t < total && lok) arena[loff + r] = r == 0 ? llo : r == 1 ? nkw : ls[r - 2];
    } else {
      if (t < total && lok) arena[loff + r] = r == 0 ? llo : r == 1 ? uint64_t(lm) : ls[r - 2];
    }
  }
}

// ---------------------------------------------------------------------------
// Single-GPU de-dup without a sort (the pair-key set of smashMEM.py:149,
// 217-228, first occurrence in pair order wins): two kernels, no LDS, so they
// run beside the next batch's search.
//
// k_dedup_claim: every keyed pair q (pair g = row_base + q of the run) walks
// the probe sequence of its hash hi.
//   * an empty slot: CAS the hi in, then store ref = g + 1, its claim;
//   * a slot holding hi whose ref names a pair of an earlier batch (a row
//     ref below row_base) or an arena record (kRefPub): same key (that row,
//     or the record, compared) -> q is a duplicate of an earlier batch; else
//     go on probing (a hash collision);
//   * a slot holding hi claimed in this batch by pair q2 (a ref from
//     row_base on): same key (q2's hit row compared) -> atomicMin the ref
//     with g + 1: the slot ends up naming the smallest pair of the batch
//     with that key; else go on probing.
//   A slot's key never changes once claimed (every pair that lowers its ref
//   has the claimer's key), so a comparison against whichever pair the ref
//   names is a comparison against the claimer.  A claim's ref is stored right
//   after its CAS; a prober that sees the hi before the ref reads the slot
//   again on its next trip.
// k_dedup_decide: pair q is kept iff its slot's ref is still its own claim
//   (the smallest pair of its key in the batch, and the key is new).  A row
//   key is done with that: the ref already names its record, and the later
//   batches see it below their row_base.  Only a kept pair of more than
//   kHitHead words writes its record into the arena and publishes the ref
//   (kRefPub: never equal to a claim, so the other pairs of the slot, reading
//   it before or after, all lose).  Fused: k_count_last's per-pair count; the
//   last major position is the post stage's (lp), cleared for a pair that
//   lost.
// slot_of[q]: the claimed slot, kSlotOld (a key of an earlier batch) or
// kSlotNone (no key, or the set is full: the error is raised).
//
// The owner's first-wins decision of the multi-GPU exchange (k_owner_claim /
// k_owner_decide) is the same scheme over the received keys: the receive
// order is the global pair order, so the smallest index j of a key is its
// first pair; every received key's record goes to the arena.  Both run
// claim_key / decide_keys below; a key source says where key j of the launch
// comes from and where a kept key's record stays.
// ---------------------------------------------------------------------------
constexpr uint64_t kSlotOld = ~0ull, kSlotNone = ~0ull - 1;
// (single GPU) slot_of flag: the pair's claim filled an empty slot.  Unless
// a later claim of the same key marked it (contest[q]), nobody else claimed
// that slot this batch, so the pair wins and k_dedup_decide skips re-reading
// the slot (one random table line per key).  Every later claimant marks the
// claim it finds (the slot's current minimum), and the first of them finds
// the filler, so a filler that lost is always marked.
constexpr uint64_t kSlotIns = 1ull << 62;

// A key source: count(j) is key j's word count (< 0: j has no key), key(j)
// the key and, on request, its hash hi; claim(j, epoch) the ref of j's claim
// and claimed(ref, epoch, j2) whether a ref is a claim of this launch, and
// whose; kMarks: its claims mark the slots they fill and the claims they
// lower (kSlotIns / contest); in_arena(m): a kept key of m words needs an
// arena record; kSamples: the key includes the sample of its pair, sample(j).
//
// the batch's pairs (single GPU): k_post's nk / hash / hit rows, which start
// at pair row_base of the run's
struct PairKeys {
  static constexpr bool kMarks = true, kSamples = false;
  const int32_t *nk;
  const uint64_t *hash;
  HitRows hits;
  uint8_t *contest;
  uint64_t row_base;
  static __device__ __forceinline__ bool in_arena(int32_t m) { return m > int32_t(kHitHead); }
  __device__ __forceinline__ unsigned long long claim(uint64_t q, uint64_t) const {
    return row_base + q + 1;
  }
  __device__ __forceinline__ bool claimed(unsigned long long ref, uint64_t, uint64_t &q2) const {
    q2 = ref - 1 - row_base;
    return (ref >> (kRefShift - 1)) == 0 && ref > row_base;
  }
  __device__ __forceinline__ int32_t count(uint64_t q) const { return nk[q]; }
  __device__ __forceinline__ KeyRef key(uint64_t q, uint64_t *hi = nullptr) const {
    if (hi) *hi = hash[2 * q];
    const int32_t k = nk[q];
    return KeyRef{hits.row(q, k), uint32_t(k), hash[2 * q + 1]};
  }
  __device__ __forceinline__ uint32_t sample(uint64_t) const { return 0; }
};

// the hash hi of a key of sample smp: the exporter and the owner of a sharded
// run must see one value; SamplePairKeys::key below holds the same expression
__device__ __forceinline__ uint64_t sample_salt(uint64_t hi, uint32_t smp, uint64_t hmask) {
  return (mix64(hi + (uint64_t(smp) + 1) * 0x9E3779B97F4A7C15ull) & hmask) | 1;
}

// the batch's pairs of a run with a sample table: PairKeys whose key includes
// the pair's sample.  The hash hi is salted with it (hmask: the post stage's
// hash mask, kept by the salted value too); lo stays the words' own, the
// sample is compared exactly beside it
struct SamplePairKeys : PairKeys {
  static constexpr bool kSamples = true;
  SampleTab tab;
  uint64_t hmask;
  __device__ __forceinline__ uint32_t sample(uint64_t q) const { return tab.of(row_base + q); }
  __device__ __forceinline__ KeyRef key(uint64_t q, uint64_t *hi = nullptr) const {
    // (sample_salt's expression, spelled out: with the call in its place
    // k_dedup_claim_smp, a kernel of the single-GPU sample run, came out with
    // other registers and one instruction fewer, and it is to keep its code)
    if (hi)
      *hi = (mix64(hash[2 * q] + (uint64_t(sample(q)) + 1) * 0x9E3779B97F4A7C15ull) & hmask) | 1;
    const int32_t k = nk[q];
    return KeyRef{hits.row(q, k), uint32_t(k), hash[2 * q + 1]};
  }
};

// an owner's received keys: header j = nk << 40 | word offset in its source
// rank's segment; base[0..world]: header prefix per source rank;
// base[65..65+world]: word prefix per source rank.  The hashes do not travel:
// they are recomputed from the words
struct RecvKeys {
  static constexpr bool kMarks = false, kSamples = false;
  const uint64_t *recv, *words, *base;
  int world;
  uint64_t hmask;
  static __device__ __forceinline__ bool in_arena(int32_t) { return true; }
  __device__ __forceinline__ unsigned long long claim(uint64_t j, uint64_t epoch) const {
    return (epoch << kRefShift) | (j + 1);
  }
  __device__ __forceinline__ bool claimed(unsigned long long ref, uint64_t epoch,
                                          uint64_t &j2) const {
    j2 = (ref & (kRefPub - 1)) - 1;
    return !(ref & kRefPub) && (ref >> kRefShift) == epoch;
  }
  __device__ __forceinline__ int32_t count(uint64_t j) const {
    return int32_t(recv[kHdrWords * j] >> 40);
  }
  __device__ __forceinline__ KeyRef key(uint64_t j, uint64_t *hi = nullptr) const {
    int r = 0;
    while (r + 1 < world && j >= base[r + 1]) ++r;
    const uint64_t nw = recv[kHdrWords * j];
    KeyRef k{words + base[65 + r] + (nw & kHdrOffMask), uint32_t(nw >> 40), 0};
    uint64_t h = 0;
    key_hashes(k.w, k.nk, hmask, h, k.lo);
    if (hi) *hi = h;
    return k;
  }
  __device__ __forceinline__ uint32_t sample(uint64_t) const { return 0; }
};

// an owner's received keys of a run with a sharded sample table
// (smash_pipeline_samples_sharded): the header has a second word, the sample
// of the key's pair, which the exporter took from the pair's global index
// (kHdrWordsSmp words per key).  The hash hi is salted with it exactly as
// SamplePairKeys salts it -- the exporter chose this owner from the same
// value -- and the sample is compared beside the words
struct RecvSampleKeys : RecvKeys {
  static constexpr bool kSamples = true;
  __device__ __forceinline__ int32_t count(uint64_t j) const {
    return int32_t(recv[kHdrWordsSmp * j] >> 40);
  }
  __device__ __forceinline__ uint32_t sample(uint64_t j) const {
    return uint32_t(recv[kHdrWordsSmp * j + 1]);
  }
  __device__ __forceinline__ KeyRef key(uint64_t j, uint64_t *hi = nullptr) const {
    int r = 0;
    while (r + 1 < world && j >= base[r + 1]) ++r;
    const uint64_t nw = recv[kHdrWordsSmp * j];
    KeyRef k{words + base[65 + r] + (nw & kHdrOffMask), uint32_t(nw >> 40), 0};
    uint64_t h = 0;
    key_hashes(k.w, k.nk, hmask, h, k.lo);
    if (hi) *hi = sample_salt(h, sample(j), hmask);
    return k;
  }
};

// The claim of key j (see above): its slot_of value.  err: the first error
// of this thread (a full set is SMASH_ERR_NOMEM).
template <class Src>
__device__ __forceinline__ uint64_t claim_key(const Src &src, uint64_t j, const KeyStore &st,
                                              uint64_t epoch, int32_t &err) {
  uint64_t *const table = st.table;
  const uint64_t mask = st.mask;
  uint64_t hi = 0;
  const KeyRef me = src.key(j, &hi);
  const unsigned long long mine = src.claim(j, epoch);
  uint32_t smp = 0;   // (kSamples) the sample every equal key must share
  if constexpr (Src::kSamples) smp = src.sample(j);
  uint64_t res = kSlotNone;
  uint64_t i = key_home(hi, mask);
  uint32_t waits = 0;
  for (uint64_t probe = 0; probe <= mask;) {
    unsigned long long *sh = reinterpret_cast<unsigned long long *>(&table[2 * i]);
    unsigned long long *sr = sh + 1;
    unsigned long long cur = __hip_atomic_load(sh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == 0) {
      const unsigned long long prev = atomicCAS(sh, 0ull, (unsigned long long)hi);
      if (prev == 0) {
        __hip_atomic_store(sr, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        res = Src::kMarks ? i | kSlotIns : i;
        break;
      }
      cur = prev;
    }
    if (cur == hi) {
      const unsigned long long ref =
          __hip_atomic_load(sr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (ref == 0) {
        // the claimer is between its CAS and its ref store: read this slot
        // again next trip (no wait inside the trip: a claimer in this wave
        // may be laid out after this branch)
        if (++waits > (1u << 22)) {   // (not a reachable state)
          err = SMASH_ERR_UNSUPPORTED;
          break;
        }
        continue;
      }
      uint64_t j2 = 0;
      if constexpr (Src::kSamples) {
        // the plain comparisons below, and the samples must agree: an arena
        // record's, a claim's pair's and a row's pair's (SamplePairKeys)
        if (ref & kRefPub) {
          if ((ref >> kRefShift) != epoch &&
              same_key(st.arena + ((ref & (kRefPub - 1)) - 1), me, smp)) {
            res = kSlotOld;
            break;
          }
        } else if (src.claimed(ref, epoch, j2)) {
          if (src.sample(j2) == smp && same_key(me, src.key(j2))) {
            if constexpr (Src::kMarks) src.contest[j2] = 1;
            atomicMin(sr, mine);
            res = i;
            break;
          }
        } else if ((ref >> kRefShift) == 0) {
          // (row refs are a pair source's: an owner's set holds arena refs only)
          if constexpr (Src::kMarks)
            if (src.tab.of(ref - 1) == smp && same_key(st, ref - 1, me)) {
              res = kSlotOld;
              break;
            }
        }
      } else if (ref & kRefPub) {
        if ((ref >> kRefShift) != epoch &&
            same_key(st.arena + ((ref & (kRefPub - 1)) - 1), me)) {
          res = kSlotOld;
          break;
        }
      } else if (src.claimed(ref, epoch, j2)) {
        if (same_key(me, src.key(j2))) {
          if constexpr (Src::kMarks) src.contest[j2] = 1;   // (see kSlotIns)
          atomicMin(sr, mine);
          res = i;
          break;
        }
      } else if ((ref >> kRefShift) == 0) {
        // a row ref of an earlier batch.  (A longer key's claim that its
        // batch could not publish, the arena full and the error raised, has
        // no record: its word count is above any row key's.)
        if (same_key(st, ref - 1, me)) {
          res = kSlotOld;
          break;
        }
      }
      // (an owner's unpublished claim of an earlier epoch: its launch ran
      // out of arena, an error already raised; no record to compare)
    }
    ++probe;
    i = (i + 1) & mask;
  }
  if (res == kSlotNone && err == 0) err = SMASH_ERR_NOMEM;   // the set is full
  return res;
}

// The decision over keys [0, n) (see above): one wave per kDecGroups x 64
// consecutive keys per trip (wave-wide scans, so every lane of a wave runs
// every trip).  The winners that need an arena record (Src::in_arena) get it
// written and their refs published -- the scans and the atomic run only in a
// wave that holds one; then item(j, win) runs for every j < n.  Returns
// whether a record of this thread did not fit the arena (SMASH_ERR_NOMEM).
template <class Src, class Item>
__device__ __forceinline__ bool decide_keys(const Src &src, uint64_t n, uint64_t *table,
                                            uint64_t *arena, uint64_t arena_cap,
                                            unsigned long long *arena_top, uint64_t epoch,
                                            const uint64_t *__restrict__ slot_of, Item item) {
  const uint64_t stride = uint64_t(gridDim.x) * blockDim.x;
  bool full = false;
  const uint32_t lane = threadIdx.x & 63;
  for (uint64_t c0 = (uint64_t(blockIdx.x) * blockDim.x + (threadIdx.x & ~63u)) * kDecGroups;
       c0 < n; c0 += stride * kDecGroups) {
    bool wins[kDecGroups];
    uint32_t needs[kDecGroups];
    bool rec = false;
#pragma unroll
    for (uint32_t g = 0; g < kDecGroups; ++g) {
      const uint64_t j = c0 + 64 * g + lane;
      const int32_t m = j < n ? src.count(j) : -1;
      bool win = false;
      if (m >= 0) {
        const uint64_t sl = slot_of[j];
        bool sole = false;                  // the slot's only claimant this batch
        if constexpr (Src::kMarks) sole = sl < kSlotNone && (sl & kSlotIns) && !src.contest[j];
        if (sole) {
          win = true;
        } else if (sl < kSlotNone) {
          const unsigned long long ref = __hip_atomic_load(
              reinterpret_cast<unsigned long long *>(&table[2 * (sl & ~kSlotIns) + 1]),
              __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          win = ref == src.claim(j, epoch);
        }
      }
      wins[g] = win;
      needs[g] = win && Src::in_arena(m) ? 2u + uint32_t(m) : 0u;
      rec = rec || needs[g];
    }
    if (__any(rec)) {   // (wave-uniform: every lane is here)
      uint32_t incls[kDecGroups], tots[kDecGroups];
      uint32_t sum = 0;
#pragma unroll
      for (uint32_t g = 0; g < kDecGroups; ++g) {
        incls[g] = wave_incl(needs[g], tots[g]);
        sum += tots[g];
      }
      unsigned long long wbase = 0;
      if (lane == 63) wbase = atomicAdd(arena_top, (unsigned long long)sum);
      wbase = __shfl(wbase, 63, 64);
#pragma unroll
      for (uint32_t g = 0; g < kDecGroups; ++g) {
        const uint64_t j = c0 + 64 * g + lane;
        const uint32_t need = needs[g], incl = incls[g], total = tots[g];
        const uint64_t off = uint64_t(wbase) + incl - need;
        wbase += total;
        const bool ok = need && off + need <= arena_cap;
        KeyRef me{nullptr, 0u, 0ull};
        if (need) me = src.key(j);
        uint32_t smp = 0;
        if constexpr (Src::kSamples) smp = need ? src.sample(j) : 0u;
        wave_fill_records<Src::kSamples>(arena, off, incl, total, ok, me.lo, me.nk, me.w, smp);
        if (need) {
          if (!ok) {
            full = true;   // the slot stays a claim: never matched (no kRefPub)
          } else {
            __hip_atomic_store(
                reinterpret_cast<unsigned long long *>(&table[2 * (slot_of[j] & ~kSlotIns) + 1]),
                (unsigned long long)((epoch << kRefShift) | kRefPub | (off + 1)),
                __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
        }
      }
    }
#pragma unroll
    for (uint32_t g = 0; g < kDecGroups; ++g) {
      const uint64_t j = c0 + 64 * g + lane;
      if (j < n) item(j, wins[g]);
    }
  }
  return full;
}

// (k_dedup_claim_smp / k_dedup_decide_smp below: the same two kernels over
// SamplePairKeys, launched when a sample table is set)
__global__ void k_dedup_claim(const int32_t *__restrict__ nk, const uint64_t *__restrict__ hash,
                              HitRows hits, uint64_t n, uint64_t row_base, KeyStore st,
                              uint64_t epoch, uint64_t *slot_of, uint8_t *contest,
                              unsigned long long *stats) {
  SMASH_BESIDE_SEARCH();
  const PairKeys src{nk, hash, hits, contest, row_base};
  const uint64_t stride = uint64_t(gridDim.x) * blockDim.x;
  int32_t err = 0;
  for (uint64_t q = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; q < n; q += stride)
    if (nk[q] >= 0) slot_of[q] = claim_key(src, q, st, epoch, err);
  if (err) atomicCAS(&stats[S_ERR], 0ull, (unsigned long long)(unsigned)err);
}

// lp: in, each pair's last major position or -1 (the post stage's); out, -1
// for the pairs that lost
__global__ void k_dedup_decide(const int32_t *__restrict__ nk, const uint64_t *__restrict__ hash,
                               HitRows hits, const uint32_t *__restrict__ nmajor, uint64_t n,
                               uint64_t row_base, uint64_t *table, uint64_t *arena,
                               uint64_t arena_cap, unsigned long long *arena_top, uint64_t epoch,
                               const uint64_t *__restrict__ slot_of,
                               const uint8_t *__restrict__ contest, uint8_t *keep,
                               uint32_t *cnt, int64_t *lp, unsigned long long *stats) {
  SMASH_BESIDE_SEARCH();
  const PairKeys src{nk, hash, hits, const_cast<uint8_t *>(contest), row_base};   // (read only here)
  unsigned long long kp = 0, dp = 0;
  const bool full = decide_keys(
      src, n, table, arena, arena_cap, arena_top, epoch, slot_of,
      [&](uint64_t q, bool win) __attribute__((always_inline)) {
        if (nk[q] >= 0) {
          ++kp;
          if (!win) {
            ++dp;
            lp[q] = -1;
          }
        }
        keep[q] = win ? 1 : 0;
        cnt[q] = win ? nmajor[q] : 0;   // k_count_last
      });
  wave_stats(stats, S_KEYPAIRS, kp, S_DUPEPAIRS, dp, full ? SMASH_ERR_NOMEM : 0);
}

__global__ void k_dedup_claim_smp(const int32_t *__restrict__ nk,
                                  const uint64_t *__restrict__ hash, HitRows hits, uint64_t n,
                                  uint64_t row_base, KeyStore st, uint64_t epoch,
                                  uint64_t *slot_of, uint8_t *contest, unsigned long long *stats,
                                  SampleTab tab, uint64_t hmask) {
  SMASH_BESIDE_SEARCH();
  const SamplePairKeys src{{nk, hash, hits, contest, row_base}, tab, hmask};
  const uint64_t stride = uint64_t(gridDim.x) * blockDim.x;
  int32_t err = 0;
  for (uint64_t q = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; q < n; q += stride)
    if (nk[q] >= 0) slot_of[q] = claim_key(src, q, st, epoch, err);
  if (err) atomicCAS(&stats[S_ERR], 0ull, (unsigned long long)(unsigned)err);
}

// (the per-sample key and duplicate counts are taken by the sample-aware emit
// kernel, which walks the pairs sample by sample; the run's totals here)
__global__ void k_dedup_decide_smp(const int32_t *__restrict__ nk,
                                   const uint64_t *__restrict__ hash, HitRows hits,
                                   const uint32_t *__restrict__ nmajor, uint64_t n,
                                   uint64_t row_base, uint64_t *table, uint64_t *arena,
                                   uint64_t arena_cap, unsigned long long *arena_top,
                                   uint64_t epoch, const uint64_t *__restrict__ slot_of,
                                   const uint8_t *__restrict__ contest, uint8_t *keep,
                                   uint32_t *cnt, int64_t *lp, unsigned long long *stats,
                                   SampleTab tab, uint64_t hmask) {
  SMASH_BESIDE_SEARCH();
  const SamplePairKeys src{{nk, hash, hits, const_cast<uint8_t *>(contest), row_base}, tab, hmask};
  unsigned long long kp = 0, dp = 0;
  const bool full = decide_keys(
      src, n, table, arena, arena_cap, arena_top, epoch, slot_of,
      [&](uint64_t q, bool win) __attribute__((always_inline)) {
        if (nk[q] >= 0) {
          ++kp;
          if (!win) {
            ++dp;
            lp[q] = -1;
          }
        }
        keep[q] = win ? 1 : 0;
        cnt[q] = win ? nmajor[q] : 0;
      });
  wave_stats(stats, S_KEYPAIRS, kp, S_DUPEPAIRS, dp, full ? SMASH_ERR_NOMEM : 0);
}

__global__ void k_owner_claim(const uint64_t *recv, const uint64_t *words, const uint64_t *base,
                              int world, uint64_t n, KeyStore st, uint64_t epoch,
                              uint64_t *slot_of, unsigned long long *stats, uint64_t hmask) {
  const RecvKeys src{recv, words, base, world, hmask};
  const uint64_t stride = uint64_t(gridDim.x) * blockDim.x;
  int32_t err = 0;
  for (uint64_t j = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; j < n; j += stride)
    slot_of[j] = claim_key(src, j, st, epoch, err);
  if (err) atomicCAS(&stats[S_ERR], 0ull, (unsigned long long)(unsigned)err);
}

__global__ void k_owner_decide(const uint64_t *recv, const uint64_t *words, const uint64_t *base,
                               int world, uint64_t n, uint64_t *table, uint64_t *arena,
                               uint64_t arena_cap, unsigned long long *arena_top, uint64_t epoch,
                               const uint64_t *__restrict__ slot_of, uint8_t *flags,
                               unsigned long long *stats, uint64_t hmask) {
  const RecvKeys src{recv, words, base, world, hmask};
  const bool full = decide_keys(src, n, table, arena, arena_cap, arena_top, epoch, slot_of,
                                [&](uint64_t j, bool win) __attribute__((always_inline)) {
                                  flags[j] = win ? 1 : 0;
                                });
  if (full) atomicCAS(&stats[S_ERR], 0ull, (unsigned long long)(unsigned)SMASH_ERR_NOMEM);
}

// the owner's two kernels over RecvSampleKeys (a sharded sample table is set)
__global__ void k_owner_claim_smp(const uint64_t *recv, const uint64_t *words,
                                  const uint64_t *base, int world, uint64_t n, KeyStore st,
                                  uint64_t epoch, uint64_t *slot_of, unsigned long long *stats,
                                  uint64_t hmask) {
  const RecvSampleKeys src{{recv, words, base, world, hmask}};
  const uint64_t stride = uint64_t(gridDim.x) * blockDim.x;
  int32_t err = 0;
  for (uint64_t j = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; j < n; j += stride)
    slot_of[j] = claim_key(src, j, st, epoch, err);
  if (err) atomicCAS(&stats[S_ERR], 0ull, (unsigned long long)(unsigned)err);
}

__global__ void k_owner_decide_smp(const uint64_t *recv, const uint64_t *words,
                                   const uint64_t *base, int world, uint64_t n, uint64_t *table,
                                   uint64_t *arena, uint64_t arena_cap,
                                   unsigned long long *arena_top, uint64_t epoch,
                                   const uint64_t *__restrict__ slot_of, uint8_t *flags,
                                   unsigned long long *stats, uint64_t hmask) {
  const RecvSampleKeys src{{recv, words, base, world, hmask}};
  const bool full = decide_keys(src, n, table, arena, arena_cap, arena_top, epoch, slot_of,
                                [&](uint64_t j, bool win) __attribute__((always_inline)) {
                                  flags[j] = win ? 1 : 0;
                                });
  if (full) atomicCAS(&stats[S_ERR], 0ull, (unsigned long long)(unsigned)SMASH_ERR_NOMEM);
}

}  // namespace
}  // namespace smash

// A key set of `keys` keys (at least the batch's max_pairs): 2x the keys in
// power-of-two slots, a head row per key (the single-GPU run's pairs), and
// the arena.  Single GPU, only the keys of more than kHitHead words go to the
// arena (C3: a few pairs in a million): one word per key of the capacity,
// a twentieth of the keys at the shortest such record.  An owner's arena
// holds every key it receives: 16 words per key (SMASH reads keep ~7 hits per
// pair, a record is 2 + nk words).
struct KeySetGeometry {
  uint64_t slots, rows, arena_words, owner_arena_words;
};
static KeySetGeometry key_set_geometry(uint64_t keys, uint64_t max_pairs) {
  const uint64_t k = std::max<uint64_t>(keys, max_pairs);
  uint64_t pw = 1;
  while (pw < 2 * k) pw <<= 1;
  return KeySetGeometry{pw, k, k + (1u << 20),
                        std::min<uint64_t>(16 * k + (1u << 20), smash::kRefPub - 2)};
}

// 1 .. 2^24 - 1, never 0 (an unpublished slot)
static uint64_t next_epoch(smash_pipeline *p) {
  p->epoch = p->epoch % ((1ull << (64 - smash::kRefShift)) - 1) + 1;
  return p->epoch;
}

// Growth of a set that holds keys: every occupied slot {hash hi, ref} of the
// old table moves to the first empty slot of its probe sequence in the new
// one (key_home, linear).  Between batches every ref names a record: a pair's
// row or an arena offset, both copied as they are, so the keys, their records
// and the first-wins decisions stay as they were; two keys with one hi take
// two slots, as they did.
__global__ void k_rehash(const uint64_t *__restrict__ old, uint64_t old_slots, uint64_t *nt,
                         uint64_t mask) {
  const uint64_t stride = uint64_t(gridDim.x) * blockDim.x;
  for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < old_slots; i += stride) {
    const uint64_t hi = old[2 * i];
    if (!hi) continue;
    uint64_t j = smash::key_home(hi, mask);
    for (uint64_t probe = 0; probe <= mask; ++probe, j = (j + 1) & mask) {
      unsigned long long *sh = reinterpret_cast<unsigned long long *>(&nt[2 * j]);
      if (atomicCAS(sh, 0ull, (unsigned long long)hi) == 0ull) {
        nt[2 * j + 1] = old[2 * i + 1];
        break;
      }
    }
  }
}
