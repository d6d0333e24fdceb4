// Top-N candidate ranking for gfx950 (MI355X): fm_rank_candidates / fm_rank_batch and their _select
// forms (include/fm_hip.h).
//
// The FM score of a context row u and a candidate row c, their entries taken together, separates:
//   yhat(u, c) = w0 + a_u + b_c + <S_u, S_c>,   a_r = b_r = L_r + (|S_r|^2 - Q_r) / 2
// with the row summaries S_r = sum v x, Q_r = sum |v|^2 x^2, L_r = sum w x that k_forward's kSummary
// mode writes in fp64 (fm_forward.hip).  Ranking is then three passes, none of which reads the table
// after the summaries:
//   k_rank_bias   a_r of every row, one fixed-order sum over f = 0 .. kp - 1;
//   k_rank_score  a block owns one context and one split of the candidates (a run of whole chunks of
//                 kRankChunk rows).  Per chunk it forms the keys -- yhat as an order-preserving 64-bit
//                 integer, the candidate row as the tie-break -- sorts the chunk in LDS (bitonic,
//                 descending) and folds its first W into the split's running best W, W the power of
//                 two that holds n_top: with A and B sorted descending, max(A[i], B[W - 1 - i]) holds
//                 the best W of both as a bitonic sequence, which one bitonic merge sorts.  The
//                 split's first n_top leave as its list;
//   k_rank_merge  a block per context folds the splits' lists in split order the same way and writes
//                 the first n_top: the candidate row, and the key's value clamped (w0 unclamped for a
//                 pair without a learned entry).
// (key, row) is a total order over a context's candidates (rows are distinct), so the best n_top and
// their order do not depend on the chunking, the splits, the context tile or the other contexts of
// the call; a score is ((w0 + a_u) + b_c) + dot with the dot product summed by one thread in the
// order f = 0 .. kp - 1, so equal rows score bit for bit alike wherever they sit.  Nothing on the
// path is rounded to fp32.
//
// Scratch: the summaries and biases, (U + C) (kp + 3) doubles and a count per row, and the split
// lists [contexts of a pass][splits][n_top] of 12 bytes, held under kRankListBudget by passing over
// the contexts in tiles (rank_ctx_tile); at most kRankMaxSplits splits, so a context's lists never
// exceed kRankMaxSplits * kRankChunk * 12 B = 768 KiB.  Nothing grows with U * C.  A call of many
// contexts takes fewer splits (rank_splits: about kRankTargetBlocks blocks in all), so its blocks
// stream several chunks each and the merge folds fewer lists.
//
// fm_rank_candidates_select / fm_rank_batch_select restrict each context to (or away from) a list of
// candidate rows: k_rank_score_sel takes k_rank_score's place between the same summaries and the
// same merge (its comment below); a list's device copy is [U + 1] offsets and the rows, 4 bytes each.
//
// fm_rank_positions / fm_rank_positions_batch count instead of sorting: k_rank_position (its comment
// below) behind the same summaries, with no split lists at all.
#include <algorithm>

#include "fm_device.h"

namespace fmhip {

namespace {

constexpr int kRankChunk = 1024;      // candidates a block scores and sorts at a time (= FM_RANK_MAX_TOP)
constexpr int kRankMaxSplits = 64;    // blocks that share one context's candidates, at most
constexpr int kRankTargetBlocks = 512;  // ... and no more than fill the chip: two blocks per CU over all contexts
constexpr int64_t kRankListBudget = 4 << 20;  // bytes of split lists in flight (one pass over a context tile)
constexpr int kRankPer = kRankChunk / kBlock;  // chunk elements per thread
static_assert(kRankChunk == FM_RANK_MAX_TOP, "a split's running list holds the largest n_top");
static_assert(kRankChunk % (2 * kBlock) == 0, "the compare-exchange loop takes whole rounds");

constexpr uint64_t kWorstKey = 0;           // below every finite score's key
constexpr uint32_t kNoRow = 0xFFFFFFFFu;    // the padding's row: after every candidate row (C < 2^31)

// yhat -> an integer whose unsigned order is yhat's (both signs; -0 was folded into +0 before)
__device__ __forceinline__ uint64_t key_of(double y) {
  const uint64_t b = (uint64_t)__double_as_longlong(y);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double value_of(uint64_t k) {
  const uint64_t b = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
  return __longlong_as_double((long long)b);
}
// (ka, ia) ranks before (kb, ib): the larger key, then the smaller row
__device__ __forceinline__ bool before(uint64_t ka, uint32_t ia, uint64_t kb, uint32_t ib) {
  return ka > kb || (ka == kb && ia < ib);
}

// One compare-exchange stage over n elements in LDS (n a power of two <= kRankChunk): partner
// distance j, blocks of kk sorted descending where (i & kk) == 0, ascending elsewhere (kk = n: all
// descending).
__device__ __forceinline__ void bitonic_stage(uint64_t* key, uint32_t* row, int j, int kk, int n) {
  for (int t = threadIdx.x; t < n / 2; t += kBlock) {
    const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
    const int l = i | j;
    const uint64_t ki = key[i], kl = key[l];
    const uint32_t ri = row[i], rl = row[l];
    const bool desc = (i & kk) == 0;
    if (before(kl, rl, ki, ri) == desc) {
      key[i] = kl; row[i] = rl;
      key[l] = ki; row[l] = ri;
    }
  }
  __syncthreads();
}
// n elements in any order (n a power of two <= kRankChunk) -> descending (the caller has synchronised
// after writing key / row)
__device__ __forceinline__ void bitonic_sort_n(uint64_t* key, uint32_t* row, int n) {
  for (int kk = 2; kk <= n; kk <<= 1)
    for (int j = kk >> 1; j > 0; j >>= 1) bitonic_stage(key, row, j, kk, n);
}
// the first W of best[] and of add[], both descending (W a power of two >= n_top) -> the first W of
// best[] = the best W of the two, descending
__device__ __forceinline__ void fold_sorted(uint64_t* bkey, uint32_t* brow, const uint64_t* akey, const uint32_t* arow,
                                            int W) {
  for (int i = threadIdx.x; i < W; i += kBlock) {
    const uint64_t ka = akey[W - 1 - i];
    const uint32_t ra = arow[W - 1 - i];
    if (before(ka, ra, bkey[i], brow[i])) {
      bkey[i] = ka;
      brow[i] = ra;
    }
  }
  __syncthreads();
  for (int j = W >> 1; j > 0; j >>= 1) bitonic_stage(bkey, brow, j, W, W);
}
// the list width of a call: the power of two that holds n_top
__device__ __forceinline__ int list_width(int n_top) {
  int W = 1;
  while (W < n_top) W <<= 1;
  return W;
}

__global__ __launch_bounds__(kBlock) void k_rank_bias(const double* __restrict__ summary, int64_t n, int kp,
                                                      double* __restrict__ bias) {
  const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (r >= n) return;
  const double2* S = reinterpret_cast<const double2*>(summary + r * kp);
  double ss = 0.0;
  for (int f = 0; f < kp / 2; ++f) {
    const double2 s = S[f];
    ss = fma(s.x, s.x, ss);
    ss = fma(s.y, s.y, ss);
  }
  const double2 ql = reinterpret_cast<const double2*>(summary + n * kp)[r];  // {Q, L}
  bias[r] = ql.y + 0.5 * (ss - ql.x);
}

// ---- what the score kernel and k_rank_position share: a block's context, a pair's key, a context's
// list of candidate rows (sel_rows / ex_rows: strictly ascending), the score a call returns.
constexpr int kSelAll = FM_RANK_SELECT_ALL, kSelOnly = FM_RANK_SELECT_ONLY, kSelExcept = FM_RANK_SELECT_EXCEPT;
constexpr int kMaskWords = kRankChunk / 32;

// A block's context u and its split s of n rows: w0 + a_u, whether u has a learned entry, and the
// split's chunks [nch s / splits, nch (s + 1) / splits) of kRankChunk rows.  (S_u goes into LDS in the
// kernel itself, one line: staged from inside a helper, k_rank_position takes 84 SGPRs for its 82.)
struct RankContext {
  double base;
  bool learned;
  int64_t ch0, ch1;
};
__device__ __forceinline__ RankContext load_context(const double* __restrict__ bias_u, const uint32_t* __restrict__ cnt_u,
                                                    int64_t u, double w0, int64_t n, int s, int splits) {
  const int64_t nch = (n + kRankChunk - 1) / kRankChunk;
  return {w0 + bias_u[u], cnt_u[u] != 0, nch * s / splits, nch * (s + 1) / splits};
}

// The key of the context (su, x) and candidate row c: ((w0 + a_u) + b_c) + dot, the dot product one
// chain over f = 0 .. kp - 1.  The only place a pair is scored.  kFreeUnroll: the loop's unrolling is
// the compiler's choice (the bits are the chain's either way).
template <bool kFreeUnroll = false>
__device__ __forceinline__ uint64_t score_row(const double* su, const RankContext& x, const double* __restrict__ sum_c,
                                              const double* __restrict__ bias_c, const uint32_t* __restrict__ cnt_c,
                                              int64_t c, int kp, double w0) {
  const double2* Sc = reinterpret_cast<const double2*>(sum_c + c * kp);
  double dot = 0.0;
  auto step = [&](int f) {
    const double2 v = Sc[f];
    dot = fma(su[2 * f], v.x, dot);
    dot = fma(su[2 * f + 1], v.y, dot);
  };
  if (kFreeUnroll) {
    // k_rank_score: more loads in flight at its 71 VGPRs (6 waves per SIMD either way)
    for (int f = 0; f < kp / 2; ++f) step(f);
  } else {
    // beside the list code, unrolled further the four rows of a thread hold 83 to 90 VGPRs (5 waves per SIMD)
#pragma unroll 2
    for (int f = 0; f < kp / 2; ++f) step(f);
  }
  double y = (x.base + bias_c[c]) + dot;
  if (!x.learned && cnt_c[c] == 0) y = w0;  // no learned entry on either side ranks at w0
  return key_of(y + 0.0);
}

// the first entry of rows[lo, hi) that is >= first (hi: none)
__device__ __forceinline__ int list_lower_bound(const int32_t* __restrict__ rows, int lo, int hi, int64_t first) {
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (rows[mid] < first) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// The chunk's 1024-bit mask (LDS) of the rows [c0, c0 + kRankChunk) that rows[cur, l1) lists, cur the
// first entry >= c0: cleared, marked (atomicOr: any order of arrival gives the same mask) and counted.
// Ascending rows make the chunk's entries one run, its length the mask's population: the return value,
// the same in every lane, is what cur moves on by.  The last reads of the mask's previous use lie before
// a barrier; this ends behind one.
__device__ __forceinline__ int mark_listed(uint32_t* mask, const int32_t* __restrict__ rows, int cur, int l1, int64_t c0) {
  const int tid = threadIdx.x;
  if (tid < kMaskWords) mask[tid] = 0;
  __syncthreads();
  for (int e = cur + tid; e < l1; e += kBlock) {
    const int64_t d = (int64_t)rows[e] - c0;
    if (d >= kRankChunk) break;
    if (d >= 0) atomicOr(&mask[d >> 5], 1u << (d & 31));
  }
  __syncthreads();
  int marked = __popc(mask[tid & (kMaskWords - 1)]);  // every 32 lanes hold the 32 words: their sum, in each lane
  for (int d = kMaskWords / 2; d > 0; d >>= 1) marked += __shfl_xor(marked, d);
  return __builtin_amdgcn_readfirstlane(marked);
}
__device__ __forceinline__ bool listed(const uint32_t* mask, int i) { return (mask[i >> 5] >> (i & 31)) & 1u; }

// The score a call returns for a pair of key `key`: globalBias unclamped for a pair without a learned
// entry (Model.scala:86), else the key's value clamped.
__device__ __forceinline__ double final_score(uint64_t key, bool learned_u, uint32_t cnt_c_of_row, double w0, double lo,
                                              double hi) {
  return learned_u || cnt_c_of_row != 0 ? fmin(fmax(value_of(key), lo), hi) : w0;
}

// The score kernel without lists.  Block b: context b / splits, split b % splits = the chunks
// [nch s / splits, nch (s + 1) / splits) of the candidates.  It stays a kernel of its own: as a third
// mode of the template below its pass measured 0.7 to 2 % slower at k = 16.
__global__ __launch_bounds__(kBlock) void k_rank_score(const double* __restrict__ sum_u, const double* __restrict__ bias_u,
                                                       const uint32_t* __restrict__ cnt_u, const double* __restrict__ sum_c,
                                                       const double* __restrict__ bias_c, const uint32_t* __restrict__ cnt_c,
                                                       int64_t C, int kp, int splits, int n_top, double w0,
                                                       uint64_t* __restrict__ lkey, uint32_t* __restrict__ lidx) {
  __shared__ double su[256];  // the context's S (kp <= 256)
  __shared__ uint64_t bkey[kRankChunk], ckey[kRankChunk];
  __shared__ uint32_t brow[kRankChunk], crow[kRankChunk];
  const int tid = threadIdx.x;
  const int64_t u = blockIdx.x / splits;
  const int s = blockIdx.x % splits;
  // load_context's values in the order this kernel has always formed them: through the helper the
  // prologue compiles to other code, and this kernel's code is held to what was measured
  const int64_t nch = (C + kRankChunk - 1) / kRankChunk;
  const int64_t ch0 = nch * s / splits, ch1 = nch * (s + 1) / splits;
  for (int f = tid; f < kp; f += kBlock) su[f] = sum_u[u * kp + f];
  const int W = list_width(n_top);
  const RankContext x = {w0 + bias_u[u], cnt_u[u] != 0, ch0, ch1};
  __syncthreads();
  for (int64_t ch = x.ch0; ch < x.ch1; ++ch) {
    uint64_t* key = ch == x.ch0 ? bkey : ckey;  // the split's first chunk is its running list
    uint32_t* row = ch == x.ch0 ? brow : crow;
#pragma unroll
    for (int j = 0; j < kRankPer; ++j) {
      const int i = tid + j * kBlock;
      const int64_t c = ch * kRankChunk + i;
      uint64_t k = kWorstKey;
      uint32_t r = kNoRow;
      if (c < C) {
        k = score_row<true>(su, x, sum_c, bias_c, cnt_c, c, kp, w0);
        r = (uint32_t)c;
      }
      key[i] = k;
      row[i] = r;
    }
    __syncthreads();
    bitonic_sort_n(key, row, kRankChunk);
    if (ch != x.ch0) fold_sorted(bkey, brow, ckey, crow, W);
  }
  const int64_t o = ((int64_t)u * splits + s) * n_top;
  for (int i = tid; i < n_top; i += kBlock) {
    lkey[o + i] = bkey[i];
    lidx[o + i] = brow[i];
  }
}

// The score kernel under per-context lists: k_rank_score's blocks, keys (score_row), sort and fold.  The
// list of context u is sel_rows[sel_ptr[u] .. sel_ptr[u + 1]), candidate rows in [0, C), strictly
// ascending (the host has checked all of it).
//   kSelExcept  the splits cut the candidates as k_rank_score's do.  The list's cursor starts at the first
//               entry >= the split's first row and moves on by the entries each chunk marks in its mask
//               (mark_listed).  A marked row enters the chunk as the padding does.
//   kSelOnly    the splits cut the chunks of the context's *list*, kRankChunk entries each; a thread
//               gathers the summaries of its listed rows and carries the candidate row as the
//               tie-break.  The split count comes from the call's longest list, so a shorter list
//               leaves splits without a chunk: those write n_top padding entries.
template <int kMode>
__global__ __launch_bounds__(kBlock) void k_rank_score_sel(const double* __restrict__ sum_u, const double* __restrict__ bias_u,
                                                           const uint32_t* __restrict__ cnt_u, const double* __restrict__ sum_c,
                                                           const double* __restrict__ bias_c, const uint32_t* __restrict__ cnt_c,
                                                           int64_t C, const int64_t* __restrict__ sel_ptr,
                                                           const int32_t* __restrict__ sel_rows, int kp, int splits, int n_top,
                                                           double w0, uint64_t* __restrict__ lkey, uint32_t* __restrict__ lidx) {
  __shared__ double su[256];  // the context's S (kp <= 256)
  __shared__ uint64_t bkey[kRankChunk], ckey[kRankChunk];
  __shared__ uint32_t brow[kRankChunk], crow[kRankChunk];
  __shared__ uint32_t mask[kMaskWords];
  const int tid = threadIdx.x;
  const int64_t u = blockIdx.x / splits;
  const int s = blockIdx.x % splits;
  const int l0 = (int)sel_ptr[u], l1 = (int)sel_ptr[u + 1];  // sel_ptr[U] < 2^31
  const int64_t n = kMode == kSelOnly ? l1 - l0 : C;  // what the splits cut: the list, or the candidates
  const RankContext x = load_context(bias_u, cnt_u, u, w0, n, s, splits);
  const int64_t o = ((int64_t)u * splits + s) * n_top;
  if (x.ch0 == x.ch1) {  // kSelOnly: no chunk of a shorter list falls into this split
    for (int i = tid; i < n_top; i += kBlock) {
      lkey[o + i] = kWorstKey;
      lidx[o + i] = kNoRow;
    }
    return;
  }
  for (int f = tid; f < kp; f += kBlock) su[f] = sum_u[u * kp + f];
  const int W = list_width(n_top);
  int cur = l0;  // kSelExcept: the first list entry at or after the chunk's first row
  if (kMode == kSelExcept) cur = list_lower_bound(sel_rows, l0, l1, x.ch0 * kRankChunk);
  __syncthreads();
  for (int64_t ch = x.ch0; ch < x.ch1; ++ch) {
    uint64_t* key = ch == x.ch0 ? bkey : ckey;  // the split's first chunk is its running list
    uint32_t* row = ch == x.ch0 ? brow : crow;
    const int64_t c0 = ch * kRankChunk;
    if (kMode == kSelExcept) cur += mark_listed(mask, sel_rows, cur, l1, c0);
#pragma unroll
    for (int j = 0; j < kRankPer; ++j) {
      const int i = tid + j * kBlock;
      uint64_t k = kWorstKey;
      uint32_t r = kNoRow;
      const int64_t c = c0 + i;
      if (c < n) {
        const int64_t cr = kMode == kSelOnly ? sel_rows[l0 + c] : c;  // the candidate row
        k = score_row(su, x, sum_c, bias_c, cnt_c, cr, kp, w0);
        r = (uint32_t)cr;
      }
      key[i] = k;
      row[i] = r;
    }
    if (kMode == kSelExcept) {
      // a listed row was scored like the rest (the scoring loop stays k_rank_score's); its owner now
      // enters it as padding
#pragma unroll
      for (int j = 0; j < kRankPer; ++j) {
        const int i = tid + j * kBlock;
        if (listed(mask, i)) {
          key[i] = kWorstKey;
          row[i] = kNoRow;
        }
      }
    }
    __syncthreads();
    bitonic_sort_n(key, row, kRankChunk);
    if (ch != x.ch0) fold_sorted(bkey, brow, ckey, crow, W);
  }
  for (int i = tid; i < n_top; i += kBlock) {
    lkey[o + i] = bkey[i];
    lidx[o + i] = brow[i];
  }
}

__global__ __launch_bounds__(kBlock) void k_rank_merge(const uint64_t* __restrict__ lkey, const uint32_t* __restrict__ lidx,
                                                       int splits, int n_top, const uint32_t* __restrict__ cnt_u,
                                                       const uint32_t* __restrict__ cnt_c, double w0, double lo, double hi,
                                                       int32_t* __restrict__ out_idx, double* __restrict__ out_score) {
  __shared__ uint64_t bkey[kRankChunk], ckey[kRankChunk];
  __shared__ uint32_t brow[kRankChunk], crow[kRankChunk];
  const int tid = threadIdx.x;
  const int64_t u = blockIdx.x;
  const int W = list_width(n_top);
  for (int s = 0; s < splits; ++s) {
    uint64_t* key = s == 0 ? bkey : ckey;
    uint32_t* row = s == 0 ? brow : crow;
    const int64_t o = (u * splits + s) * n_top;
    for (int i = tid; i < W; i += kBlock) {  // a list is descending; the padding follows it
      key[i] = i < n_top ? lkey[o + i] : kWorstKey;
      row[i] = i < n_top ? lidx[o + i] : kNoRow;
    }
    __syncthreads();
    if (s != 0) fold_sorted(bkey, brow, ckey, crow, W);
  }
  const bool learned_u = cnt_u[u] != 0;
  for (int i = tid; i < n_top; i += kBlock) {
    const uint32_t c = brow[i];
    // padding: fewer eligible rows than n_top (the _select calls), row -1 and NaN
    out_idx[u * n_top + i] = (int32_t)c;
    out_score[u * n_top + i] = c == kNoRow ? __longlong_as_double(0x7FF8000000000000ll)
                                           : final_score(bkey[i], learned_u, cnt_c[c], w0, lo, hi);
  }
}

// ---- exact positions (fm_rank_positions / fm_rank_positions_batch).  The position of a target row t
// of context u among u's eligible rows is a count, #{eligible c : (key(u, c), c) before (key(u, t), t)},
// so nothing is sorted but the targets themselves, once per block.
//
// Block (x, y): context y of the launch; x = tile * splits + s, tile a run of kRankChunk of the
// context's targets (tgt_rows[tgt_ptr[u] ..), strictly ascending), s a split of the candidate chunks cut
// as k_rank_score's.  A context with fewer tiles leaves its further blocks without work.
//   prologue  the tile's keys by score_row (the bits the ranking kernels sort), each with its index in
//             the tile as the tie-break -- the rows of a list ascend, so among targets the index orders
//             as the row does -- sorted descending over the power of two that holds them; the padding
//             sorts last.  lrow keeps the rows by index for the compare with a candidate.
//   chunks    the exclude list enters as k_rank_score_sel's kSelExcept does (two masks in turn, so a
//             chunk's mask is cleared while the last one is still read).  An eligible row finds by
//             binary search the first sorted target it ranks before: it beats that one and all behind
//             it, and not itself.  p = 0 (all of them) is counted in a register, p = m (none) not at
//             all, the rest by an integer LDS atomic on hist[p]: any order of arrival, the same counts.
//   epilogue  the inclusive prefix sum of hist is each sorted target's count in this split.  The
//             splits add theirs onto the zeroed output with an integer atomic; split 0 writes the
//             score.  A target found in the context's own exclude list gets -1 / NaN from split 0 and
//             no count from anyone.
constexpr int kPosCtxTile = 65535;  // contexts of one launch: the grid's y extent

__global__ __launch_bounds__(kBlock) void k_rank_position(
    const double* __restrict__ sum_u, const double* __restrict__ bias_u, const uint32_t* __restrict__ cnt_u,
    const double* __restrict__ sum_c, const double* __restrict__ bias_c, const uint32_t* __restrict__ cnt_c, int64_t C,
    const int64_t* __restrict__ tgt_ptr, const int32_t* __restrict__ tgt_rows, const int64_t* __restrict__ ex_ptr,
    const int32_t* __restrict__ ex_rows, int kp, int splits, double w0, double lo, double hi, int32_t* __restrict__ position,
    double* __restrict__ score) {
  __shared__ double su[256];  // the context's S (kp <= 256)
  __shared__ uint64_t tkey[kRankChunk];   // the tile's keys, sorted descending
  __shared__ uint32_t tidx[kRankChunk];   // ... and each one's index in the tile
  __shared__ uint32_t lrow[kRankChunk];   // the tile's candidate rows by index
  __shared__ uint32_t hist[kRankChunk];   // hist[p]: rows whose first beaten target is sorted entry p
  __shared__ uint32_t mask[2][kMaskWords];
  __shared__ uint32_t wsum[kBlock / 64];
  const int tid = threadIdx.x;
  const int64_t u = blockIdx.y;
  const int tile = blockIdx.x / splits, s = blockIdx.x % splits;
  const int64_t t0 = tgt_ptr[u] + (int64_t)tile * kRankChunk;
  if (t0 >= tgt_ptr[u + 1]) return;  // the whole block: a context with fewer targets than the call's longest list
  const int m = tgt_ptr[u + 1] - t0 < kRankChunk ? (int)(tgt_ptr[u + 1] - t0) : kRankChunk;
  int n = 1;
  while (n < m) n <<= 1;
  const bool ex = ex_ptr != nullptr;
  const int l0 = ex ? (int)ex_ptr[u] : 0, l1 = ex ? (int)ex_ptr[u + 1] : 0;  // ex_ptr[U] < 2^31
  const RankContext x = load_context(bias_u, cnt_u, u, w0, C, s, splits);
  for (int f = tid; f < kp; f += kBlock) su[f] = sum_u[u * kp + f];
  __syncthreads();
  for (int i = tid; i < kRankChunk; i += kBlock) {
    uint64_t k = kWorstKey;
    uint32_t xi = kNoRow;
    if (i < m) {
      const uint32_t r = (uint32_t)tgt_rows[t0 + i];
      lrow[i] = r;
      k = score_row(su, x, sum_c, bias_c, cnt_c, r, kp, w0);
      xi = (uint32_t)i;
    }
    tkey[i] = k;
    tidx[i] = xi;
    hist[i] = 0;
  }
  __syncthreads();
  bitonic_sort_n(tkey, tidx, n);

  int cur = l0;  // the first exclude entry at or after the chunk's first row
  if (ex) cur = list_lower_bound(ex_rows, l0, l1, x.ch0 * kRankChunk);
  uint32_t all = 0;  // rows of this thread that rank before every target of the tile
  for (int64_t ch = x.ch0; ch < x.ch1; ++ch) {
    const int64_t c0 = ch * kRankChunk;
    uint32_t* mk = mask[(ch - x.ch0) & 1];
    if (ex) cur += mark_listed(mk, ex_rows, cur, l1, c0);
    uint64_t key[kRankPer];
    bool live[kRankPer];
#pragma unroll
    for (int j = 0; j < kRankPer; ++j) {
      const int i = tid + j * kBlock;
      const int64_t c = c0 + i;
      live[j] = c < C && !(ex && listed(mk, i));
      key[j] = live[j] ? score_row(su, x, sum_c, bias_c, cnt_c, c, kp, w0) : kWorstKey;
    }
#pragma unroll
    for (int j = 0; j < kRankPer; ++j) {
      if (!live[j]) continue;
      const uint32_t c = (uint32_t)(c0 + tid + j * kBlock);
      int p = 0, q = m;  // the first sorted target in [0, m) that (key, c) ranks before; m: none
      while (p < q) {
        const int mid = (p + q) >> 1;
        const uint64_t kt = tkey[mid];
        if (key[j] > kt || (key[j] == kt && c < lrow[tidx[mid]])) q = mid; else p = mid + 1;
      }
      if (p == 0) ++all;
      else if (p < m) atomicAdd(&hist[p], 1u);
    }
  }
  for (int d = 32; d > 0; d >>= 1) all += __shfl_xor(all, d);
  if ((tid & 63) == 0 && all) atomicAdd(&hist[0], all);
  __syncthreads();

  // inclusive prefix sum of hist: entry i of the sorted tile is beaten by count(i) rows of this split
  uint32_t h[kRankPer], run = 0;
#pragma unroll
  for (int j = 0; j < kRankPer; ++j) {
    run += hist[tid * kRankPer + j];
    h[j] = run;
  }
  uint32_t scan = run;
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t y = __shfl_up(scan, d);
    if ((tid & 63) >= d) scan += y;
  }
  if ((tid & 63) == 63) wsum[tid >> 6] = scan;
  __syncthreads();
  uint32_t off = scan - run;
  for (int wv = 0; wv < (tid >> 6); ++wv) off += wsum[wv];
#pragma unroll
  for (int j = 0; j < kRankPer; ++j) {
    const int i = tid * kRankPer + j;
    if (i >= m) continue;  // the padding sorted behind the m targets
    const uint32_t x_t = tidx[i];
    const uint32_t r = lrow[x_t];
    bool out = false;  // the target is on the context's own exclude list
    if (ex) {
      const int a = list_lower_bound(ex_rows, l0, l1, r);
      out = a < l1 && (uint32_t)ex_rows[a] == r;
    }
    const int64_t e = t0 + x_t;
    if (out) {
      if (s == 0) {
        position[e] = -1;
        score[e] = __longlong_as_double(0x7FF8000000000000ll);
      }
      continue;
    }
    const uint32_t count = off + h[j];
    if (count) atomicAdd(&position[e], (int32_t)count);
    if (s == 0) score[e] = final_score(tkey[i], x.learned, cnt_c[r], w0, lo, hi);
  }
}

}  // namespace

int64_t rank_position_ctx_tile() { return kPosCtxTile; }

void launch_rank_position(const RankSide& u, const RankSide& c, const int64_t* tgt_ptr, const int32_t* tgt_rows,
                          int64_t longest, const int64_t* ex_ptr, const int32_t* ex_rows, int kp, int splits, double w0,
                          double lo, double hi, int32_t* position, double* score, hipStream_t st) {
  FM_REQUIRE(kp <= 256, "dimFactorization > 256 is not supported");
  FM_REQUIRE(u.n >= 1 && u.n <= kPosCtxTile && c.n >= 1 && c.n < (int64_t(1) << 31) && longest >= 1 && longest <= c.n,
             "rank positions: bad shape");
  FM_REQUIRE(splits >= 1 && splits <= kRankMaxSplits && splits <= (c.n + kRankChunk - 1) / kRankChunk,
             "rank positions: every split needs a chunk");
  const int64_t tiles = (longest + kRankChunk - 1) / kRankChunk;  // < 2^21, times splits <= 64: below 2^31
  hipLaunchKernelGGL(k_rank_position, dim3((unsigned)(tiles * splits), (unsigned)u.n), dim3(kBlock), 0, st, u.sum, u.bias,
                     u.cnt, c.sum, c.bias, c.cnt, c.n, tgt_ptr, tgt_rows, ex_ptr, ex_rows, kp, splits, w0, lo, hi, position,
                     score);
  FM_HIP_CHECK(hipGetLastError());
}

int rank_splits(int64_t C, int64_t U) {
  const int64_t nch = (C + kRankChunk - 1) / kRankChunk;
  const int64_t want = (kRankTargetBlocks + (U < 1 ? 1 : U) - 1) / (U < 1 ? 1 : U);
  const int64_t s = std::min<int64_t>(std::min<int64_t>(nch, kRankMaxSplits), want);
  return (int)(s < 1 ? 1 : s);
}

int64_t rank_ctx_tile(int splits, int n_top) {
  const int64_t per_ctx = (int64_t)splits * n_top * (int64_t)(sizeof(uint64_t) + sizeof(uint32_t));
  const int64_t t = kRankListBudget / per_ctx;
  return t < 1 ? 1 : t;
}

void launch_rank_bias(const double* summary, int64_t n, int kp, double* bias, hipStream_t st) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_rank_bias, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, summary, n, kp, bias);
  FM_HIP_CHECK(hipGetLastError());
}

void launch_rank_score(int select, const RankSide& u, const RankSide& c, const int64_t* sel_ptr, const int32_t* sel_rows,
                       int kp, int splits, int n_top, double w0, uint64_t* lkey, uint32_t* lidx, hipStream_t st) {
  FM_REQUIRE(kp <= 256, "dimFactorization > 256 is not supported");
  FM_REQUIRE(select == kSelAll || select == kSelOnly || select == kSelExcept, "rank: bad select");
  FM_REQUIRE(u.n >= 1 && c.n >= 1 && n_top >= 1 && n_top <= kRankChunk && n_top <= c.n, "rank: bad shape");
  FM_REQUIRE(splits >= 1 && splits <= kRankMaxSplits, "rank: bad split count");
  FM_REQUIRE(select == kSelOnly || splits <= (c.n + kRankChunk - 1) / kRankChunk, "rank: every split needs a chunk");
  FM_REQUIRE(u.n * splits < (int64_t(1) << 31), "rank: context tile too large");
  const dim3 grid((unsigned)(u.n * splits)), block(kBlock);
  if (select == kSelAll)
    hipLaunchKernelGGL(k_rank_score, grid, block, 0, st, u.sum, u.bias, u.cnt, c.sum, c.bias, c.cnt, c.n, kp, splits, n_top, w0,
                       lkey, lidx);
  else
    hipLaunchKernelGGL(select == kSelOnly ? k_rank_score_sel<kSelOnly> : k_rank_score_sel<kSelExcept>, grid, block, 0, st, u.sum,
                       u.bias, u.cnt, c.sum, c.bias, c.cnt, c.n, sel_ptr, sel_rows, kp, splits, n_top, w0, lkey, lidx);
  FM_HIP_CHECK(hipGetLastError());
}

void launch_rank_merge(const uint64_t* lkey, const uint32_t* lidx, int64_t Ut, int splits, int n_top, const uint32_t* cnt_u,
                       const uint32_t* cnt_c, double w0, double lo, double hi, int32_t* out_idx, double* out_score,
                       hipStream_t st) {
  FM_REQUIRE(Ut >= 1 && Ut < (int64_t(1) << 31) && splits >= 1 && n_top >= 1 && n_top <= kRankChunk, "rank: bad shape");
  hipLaunchKernelGGL(k_rank_merge, dim3((unsigned)Ut), dim3(kBlock), 0, st, lkey, lidx, splits, n_top, cnt_u, cnt_c, w0, lo,
                     hi, out_idx, out_score);
  FM_HIP_CHECK(hipGetLastError());
}

}  // namespace fmhip
