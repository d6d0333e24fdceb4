// Row-sharded FM SGD step, owner-computes (one context per rank; the owner of feature id is
// id % R, its local slot id / R).  Every rank holds 1/R of the table and steps its own
// mini-batch.  One iteration is five phases of the C-ABI joined by three all-to-alls; the
// first two depend on the batch alone and run one iteration ahead on the side stream:
//
//   fm_shard_route          requester: per sample the owners it touches and the pair index of
//                           every (sample, owner) pair; the entries partitioned by owner (CSR
//                           order kept) as {slot} and {pair index within the owner's block, x}
//                           by one stable radix pass over owner bits above the slot   [side]
//   -- all-to-all entries -->
//   fm_shard_owner_prepare  owner: the received entries' pair table (pair = source offset + the
//                           carried local index; one pass) and their stable order by slot
//                           (source rank, then CSR order)                               [side]
//   fm_shard_owner_forward  owner: per received pair, the partial forward sums over the entries
//                           it owns: [sum v*x | sum v^2 x^2 | sum w*x], lazy L1 caught up on read
//                           (FactorizationMachinesModel.scala:173-221)                [main]
//   -- all-to-all partials <--
//   fm_shard_combine        requester: per sample, the owners' partials summed in owner order
//                           (fp64) -> vfxiSum S, yhat, loss; S | yhat | y sent back per pair
//   -- all-to-all S -->
//   fm_shard_owner_update   owner: the fused segmented gradient + update + L1 of fm_update.hip
//                           (SGD.scala:143-181) over the slot-sorted entries, on its own rows
//
// Semantics equal the single-table step over the ranks' batches concatenated in rank order
// (global miniBatchSize m = sum of the ranks' rows), up to fp summation order: the forward
// sums are split per owner (fp32 on the wire; with fm_config.wire = FM_WIRE_FP64 the shares cross
// unrounded, so a sample's sums are fp64 over all of its entries, as the single table's), the
// per-feature gradient sums run over the same entries in the same order.  Deterministic for a given R.
// Traffic per rank and step (k = 16, z = 39, R = 8): entries 12 B each (off the critical path:
// exchanged during the previous iteration), partials and S (kp + 2) * 4 B per (sample, owner)
// pair -- about 2 x 150 MB, against about 1 GB when rows and gradients of every distinct id
// travel instead.
// Wire buffers are structures of arrays over the pairs, so every k-vector is 16-B aligned and a
// 64-B row at k = 16: partials [P][kp] fp32 sum v*x then [P] fp32 {sum v^2 x^2, sum w x}; S [P][kp]
// fp32 vfxiSum then [P] fp32 {r, yhat} (r = yhat - y formed in fp64 by the requester, then rounded).
// FM_WIRE_FP64: the partials' words are fp64 (a 128-B row at k = 16, the scalars a double2); S is unchanged.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "fm_context.h"
#include "fm_device.h"

namespace fmhip {

namespace {

constexpr int kMaxR = 64;     // owner masks are uint64
// the most blocks of the streaming kernels here (k_sample_mask, k_route_keys, k_key_slots, k_pair_table,
// k_pack_srec): beyond it a block takes further sweeps.  The launches and shard_geometry both read it.
constexpr int64_t kShardGrid = 256 * 16;

__device__ __forceinline__ uint32_t incl_scan_u32(uint32_t v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(v, o);
    if (lane >= o) v += t;
  }
  return v;
}

// ------------------------------------------------------------------ requester: route
constexpr int kTeamR = 16;  // lanes per sample in the route kernels (coalesced entry reads)

__device__ __forceinline__ uint64_t team_or64(uint64_t m) {
  uint32_t lo = (uint32_t)m, hi = (uint32_t)(m >> 32);
#pragma unroll
  for (int o = 1; o < kTeamR; o <<= 1) {
    lo |= __shfl_xor(lo, o);
    hi |= __shfl_xor(hi, o);
  }
  return ((uint64_t)hi << 32) | lo;
}

// per sample (a team of lanes over its entries): the owners it touches (bit mask); per owner:
// entry counts.  Ids >= F (a predict batch's ids outside the model, dropped by the inner joins of
// Model.scala:103-112) belong to no owner.
__global__ __launch_bounds__(kBlock) void k_sample_mask(const int64_t* __restrict__ row_ptr,
                                                        const uint32_t* __restrict__ col, int64_t B, uint32_t R,
                                                        uint64_t F, uint64_t* __restrict__ mask,
                                                        unsigned long long* __restrict__ ecount) {
  constexpr int TPB = kBlock / kTeamR;
  __shared__ uint32_t cnt[kMaxR];
  if (threadIdx.x < kMaxR) cnt[threadIdx.x] = 0;
  __syncthreads();
  const int tl = threadIdx.x % kTeamR;
  for (int64_t s0 = (int64_t)blockIdx.x * TPB; s0 < B; s0 += (int64_t)gridDim.x * TPB) {  // block-uniform
    const int64_t s = s0 + threadIdx.x / kTeamR;
    uint64_t m = 0;
    if (s < B) {
      for (int64_t e = row_ptr[s] + tl; e < row_ptr[s + 1]; e += kTeamR) {
        if (col[e] >= F) continue;
        const uint32_t o = col[e] % R;
        m |= 1ull << o;
        atomicAdd(&cnt[o], 1u);
      }
    }
    m = team_or64(m);
    if (s < B && tl == 0) mask[s] = m;
  }
  __syncthreads();
  if (threadIdx.x < R && cnt[threadIdx.x]) atomicAdd(&ecount[threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
}

// per entry, in CSR order: key = owner << sb | slot and the wire payload {pair index of (sample,
// owner) within the owner's block, x bits}, so one stable pass over the owner bits lays out the
// send buffers.  Ids >= F get owner R: they sort after every owner's block and are not sent.  One
// lane per entry: the exploded entry {sample, x} names its sample, so the pass streams the id and
// entry arrays without the CSR row walk (neighbouring lanes share a sample's pair indices).
constexpr int kRkU = 4;  // entries a thread takes per sweep
__global__ __launch_bounds__(kBlock) void k_route_keys(const uint32_t* __restrict__ col, const uint2* __restrict__ ent,
                                                       int64_t N, uint32_t R, int sb, uint64_t F,
                                                       const int32_t* __restrict__ pairidx, uint32_t* __restrict__ key,
                                                       uint2* __restrict__ pay) {
  // kRkU entries per thread at once: their ids and entries, then their pair indices, each a single
  // round trip (clamped indices)
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t e0 = (int64_t)blockIdx.x * kBlock + threadIdx.x; e0 < N; e0 += kRkU * stride) {
    uint32_t id[kRkU];
    uint2 en[kRkU];
#pragma unroll
    for (int u = 0; u < kRkU; ++u) {
      const int64_t e = e0 + u * stride;
      const int64_t ec = e < N ? e : N - 1;
      id[u] = col[ec];
      en[u] = ent[ec];
    }
    int32_t px[kRkU];
#pragma unroll
    for (int u = 0; u < kRkU; ++u) {
      const uint32_t o = id[u] < F ? id[u] % R : 0u;
      px[u] = pairidx[(int64_t)en[u].x * R + o];
    }
#pragma unroll
    for (int u = 0; u < kRkU; ++u) {
      const int64_t e = e0 + u * stride;
      if (e >= N) break;
      if (id[u] >= F) {
        key[e] = R << sb;
        pay[e] = make_uint2(0u, en[u].y);
        continue;
      }
      const uint32_t o = id[u] % R;
      key[e] = (o << sb) | (id[u] / R);
      pay[e] = make_uint2((uint32_t)px[u], en[u].y);
    }
  }
}

// The owner's received S rows, wire layout [P][kp] vectors then [P] {r, yhat} -> the single-table
// step's per-sample records [P][rec] = [S (kp) | {r, yhat} | 0 pad] (kp <= 16: 64- or 128-B
// records), so the segmented update gathers one line per entry instead of two (the S row and its
// scalars).  Streaming, float4 per lane.
__global__ __launch_bounds__(kBlock) void k_pack_srec(const float* __restrict__ vec, const float2* __restrict__ sc,
                                                      int64_t P, int kp, int rec, float* __restrict__ out) {
  const int q = rec / 4;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < P * q; i += (int64_t)gridDim.x * kBlock) {
    const int64_t pr = i / q;
    const int j = (int)(i - pr * q) * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (j < kp) {
      v = *reinterpret_cast<const float4*>(vec + pr * kp + j);
    } else if (j == kp) {
      const float2 s2 = sc[pr];
      v.x = s2.x;
      v.y = s2.y;
    }
    *reinterpret_cast<float4*>(out + pr * rec + j) = v;
  }
}

__global__ void k_key_slots(const uint32_t* __restrict__ key, int64_t n, uint32_t slot_mask,
                            uint32_t* __restrict__ slot) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    slot[i] = key[i] & slot_mask;
}

// pairs per (owner, tile of kBlock samples) -> tcnt[o][tile]
__global__ __launch_bounds__(kBlock) void k_pair_count(const uint64_t* __restrict__ mask, int64_t B, int R,
                                                       int64_t ntiles, uint32_t* __restrict__ tcnt) {
  __shared__ uint32_t wc[kBlock / 64][kMaxR];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint64_t m = s < B ? mask[s] : 0ull;
  for (int o = 0; o < R; ++o) {
    const uint64_t b = __ballot((m >> o) & 1ull);
    if (lane == 0) wc[wave][o] = (uint32_t)__popcll(b);
  }
  __syncthreads();
  if (threadIdx.x < R) {
    uint32_t t = 0;
    for (int w = 0; w < kBlock / 64; ++w) t += wc[w][threadIdx.x];
    tcnt[(int64_t)threadIdx.x * ntiles + blockIdx.x] = t;
  }
}

// one block per row: exclusive scan of rows[r][0..n) in place, row total -> tot[r]
__global__ __launch_bounds__(kBlock) void k_rows_scan(uint32_t* __restrict__ rows, int64_t n,
                                                      unsigned long long* __restrict__ tot) {
  __shared__ uint32_t ws[kBlock / 64];
  uint32_t* row = rows + (int64_t)blockIdx.x * n;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t carry = 0;
  for (int64_t b = 0; b < n; b += kBlock) {
    const int64_t i = b + threadIdx.x;
    const uint32_t v = i < n ? row[i] : 0u;
    const uint32_t inc = incl_scan_u32(v, lane);
    if (lane == 63) ws[wave] = inc;
    __syncthreads();
    uint32_t pre = 0, t = 0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) {
      pre += w < wave ? ws[w] : 0u;
      t += ws[w];
    }
    if (i < n) row[i] = carry + pre + inc - v;
    carry += t;
    __syncthreads();
  }
  if (threadIdx.x == 0) tot[blockIdx.x] = carry;
}

// pair index of every (sample, owner): owner o's pairs are numbered in sample order
__global__ __launch_bounds__(kBlock) void k_pair_index(const uint64_t* __restrict__ mask, int64_t B, int R,
                                                       int64_t ntiles, const uint32_t* __restrict__ toff,
                                                       int32_t* __restrict__ pairidx) {
  __shared__ uint32_t wc[kBlock / 64][kMaxR];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint64_t m = s < B ? mask[s] : 0ull;
  const uint64_t lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  for (int o = 0; o < R; ++o) {
    const uint64_t b = __ballot((m >> o) & 1ull);
    if (lane == 0) wc[wave][o] = (uint32_t)__popcll(b);
  }
  __syncthreads();
  for (int o = 0; o < R; ++o) {
    const bool bit = (m >> o) & 1ull;
    const uint64_t b = __ballot(bit);
    uint32_t pre = toff[(int64_t)o * ntiles + blockIdx.x] + (uint32_t)__popcll(b & lt);
    for (int w = 0; w < wave; ++w) pre += wc[w][o];
    if (s < B) pairidx[s * R + o] = bit ? (int32_t)pre : -1;
  }
}

// ------------------------------------------------------------------ owner: pairs
// The received entries are source-major, each source's in its CSR order, carrying their pair's
// index within that source's block: ent2 = {pair = pbase[source] + local, x}, and the first
// entry of every pair opens it in pair_ptr (one pass, no scan).
// ent2 == nullptr (one source: its pairs start at 0, so ent2 would equal ent): the pair table only.
constexpr int kPtU = 4;  // entries a thread takes per sweep
__global__ __launch_bounds__(kBlock) void k_pair_table(const uint2* __restrict__ ent, int64_t n,
                                                       const int64_t* __restrict__ src_off,
                                                       const int64_t* __restrict__ pbase, int R,
                                                       int64_t* __restrict__ pair_ptr, uint2* __restrict__ ent2) {
  // the source offsets and pair bases in LDS (a loop of dependent global loads per entry otherwise);
  // an entry and its predecessor loaded together (clamped index), kPtU entries per thread at once
  __shared__ int64_t so[kMaxR + 1], pb[kMaxR];
  for (int t = threadIdx.x; t <= R; t += kBlock) so[t] = src_off[t];
  for (int t = threadIdx.x; t < R; t += kBlock) pb[t] = pbase[t];
  __syncthreads();
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i0 = (int64_t)blockIdx.x * kBlock + threadIdx.x; i0 < n; i0 += kPtU * stride) {
    uint2 e[kPtU];
    uint32_t px[kPtU];
#pragma unroll
    for (int u = 0; u < kPtU; ++u) {
      const int64_t i = i0 + u * stride;
      const int64_t ic = i < n ? i : n - 1;
      e[u] = ent[ic];
      px[u] = ent[ic > 0 ? ic - 1 : 0].x;
    }
#pragma unroll
    for (int u = 0; u < kPtU; ++u) {
      const int64_t i = i0 + u * stride;
      if (i >= n) break;
      int r = 0;
      while (r + 1 < R && so[r + 1] <= i) ++r;
      const uint32_t pair = (uint32_t)pb[r] + e[u].x;
      if (ent2) ent2[i] = make_uint2(pair, e[u].y);
      if (i == so[r] || px[u] != e[u].x) pair_ptr[pair] = i;
    }
  }
}

// ------------------------------------------------------------------ requester: combine, predict
// The partial direction's element type W: float (FM_WIRE_FP32) or double (FM_WIRE_FP64).
template <typename W>
using wire2 = std::conditional_t<std::is_same<W, double>::value, double2, float2>;

// What a requester kernel reads of the partials.  Wire layout (structure of arrays): vec [pair][kp]
// sum v*x, sc [pair] {sum v^2 x^2, sum w x}; the sample's pair at owner o is poff[o] + pairidx[s * R + o]
// (-1: none).
template <typename W>
struct ReqIn {
  const int64_t* poff;
  const W* vec;
  const wire2<W>* sc;
  int kp;
  double w0;
};

// The two ways of reaching a sample's rows in the owners' blocks.
//
// Owner by owner (OwnerWalk, any R up to kMaxR): guarded loads, one per owner, each waited out its
// round trip before the next: 2R + R round trips per sample and quad.
//
// Slots in registers (int64_t pj[OW], R <= OW owners; -1: no pair): every owner's loads of a pass
// are issued before any is used (clamped owner indices; a pair the sample lacks reads poff's first
// bytes and is masked out; poff is allocated at least 32 B so every masked load, 16 B at the most,
// stays inside it).  W = double: an owner's quad is loaded as two double2 halves, one half of every
// owner at a time, so the loads in flight take the registers the fp32 quads take.  pj stays a local
// array of the kernel and the helpers are free functions over a reference to it (as members of a
// struct holding pj the same code took up to 26 VGPRs more and a wave per SIMD: DESIGN.md §5).
struct OwnerWalk {
  const int32_t* pi;  // the sample's row of pairidx
  const int64_t* poff;
  int R;
};

template <int OW>
__device__ __forceinline__ void load_slots(int64_t (&pj)[OW], const int32_t* pi, const int64_t* poff, int R) {
  int32_t ix[OW];
#pragma unroll
  for (int o = 0; o < OW; ++o) {
    const int oc = o < R ? o : R - 1;
    ix[o] = pi[oc];
    pj[o] = poff[oc];
  }
#pragma unroll
  for (int o = 0; o < OW; ++o) pj[o] = o < R && ix[o] >= 0 ? pj[o] + ix[o] : -1;
}

// f(pair) for every pair of the sample, in owner order
template <typename F>
__device__ __forceinline__ void for_each_pair(const OwnerWalk& s, F&& f) {
  for (int o = 0; o < s.R; ++o) {
    const int32_t ix = s.pi[o];
    if (ix >= 0) f(s.poff[o] + ix);
  }
}
template <int OW, typename F>
__device__ __forceinline__ void for_each_pair(const int64_t (&pj)[OW], F&& f) {
#pragma unroll
  for (int o = 0; o < OW; ++o)
    if (pj[o] >= 0) f(pj[o]);
}

// The sample's scalar sums over its owners in owner order, fp64, and n: its pairs (kCombine), or its
// present entries (pcnt [pair]: the owner's present rows among the pair's entries).
template <bool kCombine, typename W>
__device__ __forceinline__ void sum_scalars(const OwnerWalk& s, const ReqIn<W>& in, const uint32_t* pcnt, double& vv,
                                            double& wx, uint32_t& n) {
  for_each_pair(s, [&](int64_t p) {
    const wire2<W> t = in.sc[p];
    vv += (double)t.x;
    wx += (double)t.y;
    n += kCombine ? 1u : pcnt[p];
  });
}
template <bool kCombine, int OW, typename W>
__device__ __forceinline__ void sum_scalars(const int64_t (&pj)[OW], const ReqIn<W>& in, const uint32_t*, double& vv,
                                            double& wx, uint32_t& n) {
  wire2<W> t[OW];
#pragma unroll
  for (int o = 0; o < OW; ++o) t[o] = *(pj[o] >= 0 ? in.sc + pj[o] : reinterpret_cast<const wire2<W>*>(in.poff));
#pragma unroll
  for (int o = 0; o < OW; ++o) {
    vv += pj[o] >= 0 ? (double)t[o].x : 0.0;
    wx += pj[o] >= 0 ? (double)t[o].y : 0.0;
    n += pj[o] >= 0;
  }
}

// Quad q of the sample's partial rows added to the lane's four fp64 column sums, owner order
// (fp64 words: two 16-B halves).
template <typename W>
__device__ __forceinline__ void sum_quad(const OwnerWalk& s, const ReqIn<W>& in, int q, double& a0, double& a1,
                                         double& a2, double& a3) {
  for_each_pair(s, [&](int64_t p) {
    const W* row = in.vec + p * in.kp;
    if constexpr (std::is_same<W, double>::value) {
      const double2 lo = reinterpret_cast<const double2*>(row)[2 * q], hi = reinterpret_cast<const double2*>(row)[2 * q + 1];
      a0 += lo.x; a1 += lo.y; a2 += hi.x; a3 += hi.y;
    } else {
      const float4 t = reinterpret_cast<const float4*>(row)[q];
      a0 += (double)t.x; a1 += (double)t.y; a2 += (double)t.z; a3 += (double)t.w;
    }
  });
}
template <int OW, typename W>
__device__ __forceinline__ void sum_quad(const int64_t (&pj)[OW], const ReqIn<W>& in, int q, double& a0, double& a1,
                                         double& a2, double& a3) {
  if constexpr (std::is_same<W, double>::value) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {  // columns 4q + 2h, 4q + 2h + 1 of every owner, owner order
      double2 tv[OW];
#pragma unroll
      for (int o = 0; o < OW; ++o)
        tv[o] = pj[o] >= 0 ? reinterpret_cast<const double2*>(in.vec + pj[o] * in.kp)[2 * q + h]
                           : *reinterpret_cast<const double2*>(in.poff);
      double b0 = 0.0, b1 = 0.0;
#pragma unroll
      for (int o = 0; o < OW; ++o) {
        const bool ok = pj[o] >= 0;
        b0 += ok ? tv[o].x : 0.0; b1 += ok ? tv[o].y : 0.0;
      }
      if (h == 0) { a0 = b0; a1 = b1; } else { a2 = b0; a3 = b1; }
    }
  } else {
    float4 tv[OW];
#pragma unroll
    for (int o = 0; o < OW; ++o)
      tv[o] = pj[o] >= 0 ? reinterpret_cast<const float4*>(in.vec + pj[o] * in.kp)[q]
                         : *reinterpret_cast<const float4*>(in.poff);
#pragma unroll
    for (int o = 0; o < OW; ++o) {
      const bool ok = pj[o] >= 0;
      a0 += ok ? (double)tv[o].x : 0.0; a1 += ok ? (double)tv[o].y : 0.0;
      a2 += ok ? (double)tv[o].z : 0.0; a3 += ok ? (double)tv[o].w : 0.0;
    }
  }
}

// One sample of a team of GS lanes (lane g: quads g, g + GS, ...): the owners' partials summed in
// owner order in fp64 -> S = vfxiSum, yhat = 0.5 (|S|^2 - sum v^2 x^2) + sum w x + w0
// (FactorizationMachinesModel.scala:221, :260-262), returned to every lane of the team.
// kCombine: S, rounded, goes to s_vec [pair][kp] for every pair of the sample.  n: see sum_scalars.
template <int GS, bool kCombine, typename W, typename Slots>
__device__ __forceinline__ double sample_yhat(const Slots& slots, const ReqIn<W>& in, int g, const uint32_t* pcnt,
                                              float* s_vec, uint32_t& n) {
  const int nq = in.kp >> 2;
  const double w0 = in.w0;
  double vv = 0.0, wx = 0.0, ss = 0.0;
  sum_scalars<kCombine>(slots, in, pcnt, vv, wx, n);
  for (int qc = 0; qc < nq; qc += GS) {
    const int q = qc + g;
    if (q >= nq) break;  // (q grows with qc)
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    sum_quad(slots, in, q, a0, a1, a2, a3);
    ss += a0 * a0 + a1 * a1 + a2 * a2 + a3 * a3;
    if constexpr (kCombine) {
      const float4 sq = make_float4((float)a0, (float)a1, (float)a2, (float)a3);
      for_each_pair(slots, [&](int64_t p) { reinterpret_cast<float4*>(s_vec + p * in.kp)[q] = sq; });
    }
  }
#pragma unroll
  for (int o = 1; o < GS; o <<= 1) ss += __shfl_xor(ss, o);
  return 0.5 * (ss - vv) + wx + w0;
}

// The combine's sample: S rows and {r, yhat} (r = yhat - y formed in fp64, then rounded) sent back to
// every owner holding entries of the sample; s_sc [pair] float2.  A sample with no pair is not
// counted in the loss (:230).
template <int GS, typename W, typename Slots>
__device__ __forceinline__ void combine_sample(const Slots& slots, const ReqIn<W>& in, int g, const double* y, float* s_vec,
                                               float2* s_sc, double& loss_acc, double& nloss) {
  uint32_t n = 0;
  const double yhat = sample_yhat<GS, true>(slots, in, g, nullptr, s_vec, n);
  if (g == 0) {
    const double d = yhat - *y;
    for_each_pair(slots, [&](int64_t p) { s_sc[p] = make_float2((float)d, (float)yhat); });  // {r, yhat}
    if (n) {
      loss_acc += d * d;
      nloss += 1.0;
    }
  }
}

// OW > 0 (R <= OW owners): the sample's pair slots in registers; OW = 0: owner by owner.
template <int GS, int OW, typename W>
__global__ __launch_bounds__(kBlock) void k_shard_combine(const int32_t* __restrict__ pairidx,
                                                          const int64_t* __restrict__ poff, int R, int64_t B,
                                                          const W* __restrict__ part_vec,
                                                          const wire2<W>* __restrict__ part_sc, int kp, double w0,
                                                          const double* __restrict__ label, float* __restrict__ s_vec,
                                                          float2* __restrict__ s_sc, double2* __restrict__ loss_part) {
  constexpr int TPB = kBlock / GS;
  const int tid = threadIdx.x, g = tid % GS;
  const ReqIn<W> in{poff, part_vec, part_sc, kp, w0};
  double loss_acc = 0.0, nloss = 0.0;
  for (int64_t s = (int64_t)blockIdx.x * TPB + tid / GS; s < B; s += (int64_t)gridDim.x * TPB) {
    const int32_t* pi = pairidx + s * R;
    if constexpr (OW > 0) {
      int64_t pj[OW];
      load_slots(pj, pi, poff, R);
      combine_sample<GS>(pj, in, g, label + s, s_vec, s_sc, loss_acc, nloss);
    } else {
      combine_sample<GS>(OwnerWalk{pi, poff, R}, in, g, label + s, s_vec, s_sc, loss_acc, nloss);
    }
  }
  block_loss_partial(loss_acc, nloss, loss_part);
}

// The same sums for FactorizationMachinesModel.predict (Model.scala:90-133) over a sharded table:
// pcnt[pair] = the owner's present rows among the pair's entries (absent ids drop out, :103-112);
// a sample with none scores globalBias unclamped (na.fill, :78-86), every other
// least(greatest(yhat, minLabel), maxLabel) (:129-132).
template <int GS, typename W>
__global__ __launch_bounds__(kBlock) void k_shard_predict(const int32_t* __restrict__ pairidx,
                                                          const int64_t* __restrict__ poff, int R, int64_t B,
                                                          const W* __restrict__ part_vec,
                                                          const wire2<W>* __restrict__ part_sc, int kp, double w0,
                                                          const uint32_t* __restrict__ pcnt, double lo, double hi,
                                                          double* __restrict__ pred) {
  constexpr int TPB = kBlock / GS;
  const int tid = threadIdx.x, g = tid % GS;
  const ReqIn<W> in{poff, part_vec, part_sc, kp, w0};
  for (int64_t s = (int64_t)blockIdx.x * TPB + tid / GS; s < B; s += (int64_t)gridDim.x * TPB) {
    uint32_t cnt = 0;
    const double yhat = sample_yhat<GS, false>(OwnerWalk{pairidx + s * R, poff, R}, in, g, pcnt, nullptr, cnt);
    if (g == 0) pred[s] = cnt == 0 ? w0 : fmin(fmax(yhat, lo), hi);
  }
}

// k_shard_predict's scores against this rank's labels, reduced (fm_evaluate* over a sharded table): each
// team's lane 0 adds its rows to its thread's record, each block leaves one record in part
// [gridDim.x][kEvalRec] (block_eval_partial), folded by launch_eval_fold; pred (optional) gets the
// score that was subtracted.
template <int GS, typename W>
__global__ __launch_bounds__(kBlock) void k_shard_evaluate(const int32_t* __restrict__ pairidx,
                                                           const int64_t* __restrict__ poff, int R, int64_t B,
                                                           const W* __restrict__ part_vec,
                                                           const wire2<W>* __restrict__ part_sc, int kp, double w0,
                                                           const uint32_t* __restrict__ pcnt, double lo, double hi,
                                                           const double* __restrict__ label, double* __restrict__ pred,
                                                           double* __restrict__ part) {
  constexpr int TPB = kBlock / GS;
  const int tid = threadIdx.x, g = tid % GS;
  const ReqIn<W> in{poff, part_vec, part_sc, kp, w0};
  EvalAcc ev;
  for (int64_t s = (int64_t)blockIdx.x * TPB + tid / GS; s < B; s += (int64_t)gridDim.x * TPB) {
    uint32_t cnt = 0;
    const double yhat = sample_yhat<GS, false>(OwnerWalk{pairidx + s * R, poff, R}, in, g, pcnt, nullptr, cnt);
    if (g == 0) {
      const double p = eval_row(ev, yhat, cnt != 0, w0, lo, hi, label[s]);
      if (pred) pred[s] = p;
    }
  }
  block_eval_partial(ev, part + (int64_t)blockIdx.x * kEvalRec);
}

inline int team_for(int nq) {
  int G = 1;
  while (G < nq && G < 16) G <<= 1;
  return G;
}

// owner blocks of the partial / S rows: poff[o] = pairs sent to owners before o
__global__ void k_owner_offsets(const unsigned long long* __restrict__ pairs, int R, int64_t* __restrict__ poff) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    int64_t acc = 0;
    for (int o = 0; o < R; ++o) {
      poff[o] = acc;
      acc += (int64_t)pairs[o];
    }
    poff[R] = acc;
  }
}

}  // namespace

// The owner partial pass of fm_shard_owner_forward; present_out (optional, [P] uint32): the pair's
// present rows (sharded predict).
void shard_owner_partials(fm_ctx* ctx, fm_batch* b, void* partials_out, uint32_t* present_out, int chunk,
                          int chunks);

}  // namespace fmhip

using namespace fmhip;

namespace {

// Owner-side step parameters (SGD.scala:121-124 with the global miniBatchSize).
StepParams shard_params(fm_ctx* ctx, int32_t t, double step_size, double reg_param, int64_t global_rows) {
  StepParams p{};
  p.n_rows = global_rows;
  p.eta = step_size / std::sqrt((double)t);  // SGD.scala:121
  p.lam = p.eta * reg_param;                 // SGD.scala:122
  p.m = (double)global_rows;
  p.scale_v = p.eta / (double)global_rows;
  p.epoch = ctx->epoch;
  p.cumE = ctx->cum_host.back();
  p.cum_next = p.cumE + p.lam;
  p.w0 = ctx->cfg.w0;
  return p;
}

// The batch's sharded state, created on first use with its events already "done".
ShardBatchState& shard_state(fm_ctx* ctx, fm_batch* b) {
  FM_REQUIRE(b != nullptr && b->owner == ctx, "batch belongs to another context");
  FM_REQUIRE(!ctx->group, "a multi-GPU context runs its sharded phases itself (fm_step / fm_step_batch)");
  FM_REQUIRE(ctx->cfg.shard_count >= 1, "bad context");
  if (!b->sh) {
    std::unique_ptr<ShardBatchState> s(new ShardBatchState());
    FM_HIP_CHECK(hipEventCreateWithFlags(&s->ready_fwd, hipEventDisableTiming));
    FM_HIP_CHECK(hipEventCreateWithFlags(&s->ready_upd, hipEventDisableTiming));
    FM_HIP_CHECK(hipEventCreateWithFlags(&s->last_use, hipEventDisableTiming));
    FM_HIP_CHECK(hipEventRecord(s->ready_fwd, ctx->side));
    FM_HIP_CHECK(hipEventRecord(s->ready_upd, ctx->side));
    FM_HIP_CHECK(hipEventRecord(s->last_use, ctx->stream));
    b->sh = std::move(s);
  }
  return *b->sh;
}

// ------------------------------------------------------------------ requester: launch
constexpr int kSlotRegs = 8;  // up to this many owners the combine keeps the sample's pair slots in registers

// The requester kernel of a wire and team width: the combine (slots in registers or owner by
// owner), the predict or the evaluation (owner by owner).  For one W and kind every instantiation
// has one type.
enum ReqKind : int { kReqCombine = 0, kReqPredict = 1, kReqEvaluate = 2 };
template <int GS, typename W, int KIND>
auto requester_kernel_g(int R) {
  if constexpr (KIND == kReqPredict) return &k_shard_predict<GS, W>;
  else if constexpr (KIND == kReqEvaluate) return &k_shard_evaluate<GS, W>;
  else return R <= kSlotRegs ? &k_shard_combine<GS, kSlotRegs, W> : &k_shard_combine<GS, 0, W>;
}
template <typename W, int KIND>
auto requester_kernel(int GS, int R) {
  switch (GS) {
    case 1: return requester_kernel_g<1, W, KIND>(R);
    case 2: return requester_kernel_g<2, W, KIND>(R);
    case 4: return requester_kernel_g<4, W, KIND>(R);
    case 8: return requester_kernel_g<8, W, KIND>(R);
    default: return requester_kernel_g<16, W, KIND>(R);
  }
}

// A wire buffer is [P][kp] vectors, then [P] scalar pairs.
template <typename Sc, typename V>
Sc* wire_scalars(V* vec, int64_t P, int kp) {
  return reinterpret_cast<Sc*>(vec ? vec + P * kp : nullptr);
}

// What the combine and the predict take from a routed batch: its pairs over all owners, the team
// width and the grid (one team per sample, at most kLossPartBlocks blocks).
struct ReqPlan {
  int R, kp, GS;
  int64_t B, Ps;
  unsigned blocks;
  const int32_t* pi;
  const int64_t* poff;
};

ReqPlan requester_plan(fm_ctx* ctx, fm_batch* b, const ShardBatchState& S) {
  FM_REQUIRE(S.route_nnz == b->dev.nnz && (int)S.pairs_out.size() == ctx->cfg.shard_count,
             "fm_shard_route must run on this batch first");
  ReqPlan q{};
  q.R = ctx->cfg.shard_count;
  q.kp = ctx->kp;
  q.GS = team_for(q.kp / 4);
  q.B = b->dev.n_rows;
  for (int o = 0; o < q.R; ++o) q.Ps += S.pairs_out[o];
  q.blocks = grid_for(q.B, kBlock / q.GS, kLossPartBlocks);
  q.pi = S.pairidx.as<int32_t>();
  q.poff = S.poff.as<int64_t>();
  return q;
}

// The combine, predict or evaluation kernel of the context's wire on the main stream; tail: the
// kernel's own arguments after the ones all take.
template <int KIND, typename... Tail>
void launch_requester(fm_ctx* ctx, const ReqPlan& q, const void* partials_in, Tail... tail) {
  auto go = [&](auto word) {
    using W = decltype(word);
    const W* vec = reinterpret_cast<const W*>(partials_in);
    auto kern = requester_kernel<W, KIND>(q.GS, q.R);
    hipLaunchKernelGGL(kern, dim3(q.blocks), dim3(kBlock), 0, ctx->stream, q.pi, q.poff, q.R, q.B, vec,
                       wire_scalars<const wire2<W>>(vec, q.Ps, q.kp), q.kp, ctx->cfg.w0, tail...);
  };
  if (ctx->cfg.wire == FM_WIRE_FP64) go(double{});
  else go(float{});
  FM_HIP_CHECK(hipGetLastError());
}

}  // namespace

extern "C" {

int fm_shard_route(fm_ctx* ctx, fm_batch* b, void* send_slot, void* send_ent, int64_t* counts) {
  return guarded(ctx, [&]() -> int {
    require_squared(ctx, "fm_shard_route");
    FM_REQUIRE(counts != nullptr, "bad arguments");
    shard_route_launch(ctx, b, send_slot, send_ent, ctx->side);
    const int R = ctx->cfg.shard_count;
    ctx->side_pinned.ensure(sizeof(unsigned long long) * 2 * R);
    FM_HIP_CHECK(hipMemcpyAsync(ctx->side_pinned.p, ctx->sh_tot.p, sizeof(unsigned long long) * 2 * R,
                                hipMemcpyDeviceToHost, ctx->side));
    FM_HIP_CHECK(hipStreamSynchronize(ctx->side));  // the side stream only: the main stream keeps running
    shard_route_finish(ctx, b, reinterpret_cast<const unsigned long long*>(ctx->side_pinned.p), counts);
    return FM_OK;
  });
}

}  // extern "C"

namespace fmhip {

// Phase 1 enqueued on the side stream, its counts left on the device in ctx->sh_tot ([R] pairs,
// then [R] entries per owner, uint64): a multi-GPU context gathers every rank's counts on the
// device and reads them back once for the whole job (fm_group.hip prefetch).
void shard_route_launch(fm_ctx* ctx, fm_batch* b, void* send_slot, void* send_ent, hipStream_t st) {
  ShardBatchState& S = shard_state(ctx, b);
  const int R = ctx->cfg.shard_count;
  FM_REQUIRE(R <= kMaxR, "the owner-computes sharded step supports at most 64 ranks");
  const int64_t B = b->dev.n_rows, N = b->dev.nnz;
  FM_REQUIRE(N == 0 || (send_slot && send_ent), "null send buffer");
  if (!st) st = ctx->side;
  // the batch's previous iteration may still read its requester state on the main stream; a batch
  // refilled by fm_batch_from_rows is routed once its gather is done
  FM_HIP_CHECK(hipStreamWaitEvent(st, S.last_use, 0));
  wait_built(b, st);
  hipEvent_t e0 = ctx->prof_begin(st);
  const int64_t ntiles = std::max<int64_t>((B + kBlock - 1) / kBlock, 1);
  ctx->sh_okey.ensure(sizeof(uint32_t) * std::max<int64_t>(N, 4) + 16);
  ctx->sh_mask.ensure(sizeof(uint64_t) * std::max<int64_t>(B, 1));
  ctx->sh_tcnt.ensure(sizeof(uint32_t) * R * ntiles);
  ctx->sh_tot.ensure(sizeof(unsigned long long) * 2 * R);
  S.pairidx.ensure(sizeof(int32_t) * std::max<int64_t>(B, 1) * R);
  // at least 32 B: the combine's masked loads read poff's first bytes (slots in registers)
  S.poff.ensure(sizeof(int64_t) * std::max(R + 1, 4));
  unsigned long long* tot = ctx->sh_tot.as<unsigned long long>();  // [R] pairs, [R] entries
  FM_HIP_CHECK(hipMemsetAsync(tot, 0, sizeof(unsigned long long) * 2 * R, st));
  const uint64_t F = (uint64_t)ctx->cfg.num_features;
  const bool drop = b->max_id >= (int64_t)F;  // a predict batch with ids outside the model
  if (B > 0) {
    hipLaunchKernelGGL(k_sample_mask, dim3(grid_for(B * kTeamR, kBlock, kShardGrid)), dim3(kBlock), 0, st, b->dev.row_ptr.as<int64_t>(),
                       b->dev.col.as<uint32_t>(), B, (uint32_t)R, F, ctx->sh_mask.as<uint64_t>(), tot + R);
    hipLaunchKernelGGL(k_pair_count, dim3((unsigned)ntiles), dim3(kBlock), 0, st, ctx->sh_mask.as<uint64_t>(), B,
                       R, ntiles, ctx->sh_tcnt.as<uint32_t>());
    hipLaunchKernelGGL(k_rows_scan, dim3((unsigned)R), dim3(kBlock), 0, st, ctx->sh_tcnt.as<uint32_t>(), ntiles,
                       tot);
    hipLaunchKernelGGL(k_pair_index, dim3((unsigned)ntiles), dim3(kBlock), 0, st, ctx->sh_mask.as<uint64_t>(), B,
                       R, ntiles, ctx->sh_tcnt.as<uint32_t>(), S.pairidx.as<int32_t>());
  }
  hipLaunchKernelGGL(k_owner_offsets, dim3(1), dim3(64), 0, st, tot, R, S.poff.as<int64_t>());
  if (N > 0) {
    // wire keys owner << sb | slot with payload {pair index within the owner's block, x}; one
    // stable pass over the owner bits partitions them (CSR order kept inside each owner).  sb
    // must hold the largest slot of ANY owner (owner 0 has the most rows), the same on every rank
    const int sb = bits_for(std::max<int64_t>((ctx->cfg.num_features - 1) / R, 1));
    const int ob = bits_for(drop ? R : R - 1);
    FM_REQUIRE(sb + ob <= 32, "route key does not fit 32 bits");
    if (R == 1 && !drop) {
      // one owner: CSR order is already the owner order and the key is the slot -- the keys and
      // payloads go straight to the send buffers, no partition pass
      hipLaunchKernelGGL(k_route_keys, dim3(grid_for(N, kBlock, kShardGrid)), dim3(kBlock), 0, st, b->dev.col.as<uint32_t>(),
                         b->dev.ent.as<uint2>(), N, (uint32_t)R, sb, F, S.pairidx.as<int32_t>(),
                         reinterpret_cast<uint32_t*>(send_slot), reinterpret_cast<uint2*>(send_ent));
    } else {
      ctx->sh_pay.ensure(sizeof(uint2) * std::max<int64_t>(N, 4) + 16);
      ctx->sh_skey.ensure(sizeof(uint32_t) * std::max<int64_t>(N, 4) + 16);
      hipLaunchKernelGGL(k_route_keys, dim3(grid_for(N, kBlock, kShardGrid)), dim3(kBlock), 0, st, b->dev.col.as<uint32_t>(),
                         b->dev.ent.as<uint2>(), N, (uint32_t)R, sb, F, S.pairidx.as<int32_t>(),
                         ctx->sh_okey.as<uint32_t>(), ctx->sh_pay.as<uint2>());
      radix_sort_pairs64_bits(ctx->route_sort, ctx->sh_okey.as<uint32_t>(), ctx->sh_pay.as<uint2>(), N, sb, sb + ob, st,
                              ctx->sh_skey.as<uint32_t>(), reinterpret_cast<uint2*>(send_ent));
      hipLaunchKernelGGL(k_key_slots, dim3(grid_for(N, kBlock, kShardGrid)), dim3(kBlock), 0, st, ctx->sh_skey.as<uint32_t>(), N,
                         (uint32_t)((sb >= 32) ? 0xFFFFFFFFu : ((1u << sb) - 1u)), reinterpret_cast<uint32_t*>(send_slot));
    }
  }
  FM_HIP_CHECK(hipGetLastError());
  ctx->prof_end("route", e0, st);
  S.route_nnz = -1;  // until shard_route_finish has the counts
}

// The host's copy of the route counts hc ([R] pairs, [R] entries) -> counts[0..R) entries and
// counts[R..2R) pairs per owner, and the batch's requester state.
void shard_route_finish(fm_ctx* ctx, fm_batch* b, const unsigned long long* hc, int64_t* counts) {
  ShardBatchState& S = shard_state(ctx, b);
  const int R = ctx->cfg.shard_count;
  const int64_t N = b->dev.nnz;
  const bool drop = b->max_id >= (int64_t)ctx->cfg.num_features;
  S.pairs_out.assign(R, 0);
  int64_t ne = 0;
  for (int o = 0; o < R; ++o) {
    counts[o] = (int64_t)hc[R + o];      // entries to owner o
    counts[R + o] = (int64_t)hc[o];      // (sample, owner) pairs to owner o
    S.pairs_out[o] = (int64_t)hc[o];
    ne += (int64_t)hc[R + o];
  }
  FM_REQUIRE(drop ? ne <= N : ne == N, "route: inconsistent entry count");
  S.route_nnz = N;
  S.combined = false;
}

}  // namespace fmhip

extern "C" {

int fm_shard_owner_prepare(fm_ctx* ctx, fm_batch* b, const void* recv_slot, const void* recv_ent, int64_t n,
                           const int64_t* src_entries, const int64_t* src_pairs) {
  return guarded(ctx, [&]() -> int {
    require_squared(ctx, "fm_shard_owner_prepare");
    ShardBatchState& S = shard_state(ctx, b);
    const int R = ctx->cfg.shard_count;
    FM_REQUIRE(n >= 0 && src_entries && src_pairs, "bad arguments");
    std::vector<int64_t> off(2 * (R + 1), 0);  // [R+1] source entry offsets, [R+1] source pair offsets
    int64_t P = 0;
    for (int r = 0; r < R; ++r) {
      FM_REQUIRE(src_entries[r] >= 0 && src_pairs[r] >= 0 && src_pairs[r] <= src_entries[r], "bad source counts");
      FM_REQUIRE(src_entries[r] == 0 || src_pairs[r] >= 1, "bad source counts");
      off[r + 1] = off[r] + src_entries[r];
      off[R + 1 + r + 1] = off[R + 1 + r] + src_pairs[r];
      P += src_pairs[r];
    }
    FM_REQUIRE(off[R] == n, "source entry counts do not add up to n");
    FM_REQUIRE(n < (int64_t(1) << 32) - 1 && P < (int64_t(1) << 32) - 1, "too many received entries");
    FM_REQUIRE(n == 0 || (recv_slot && recv_ent), "null buffer");
    hipStream_t st = ctx->side;
    FM_HIP_CHECK(hipStreamWaitEvent(st, S.last_use, 0));
    // the staging of this batch's previous preparation has been consumed once its pair table was
    FM_HIP_CHECK(hipEventSynchronize(S.ready_fwd));
    hipEvent_t e0 = ctx->prof_begin(st);
    S.src_off.ensure(sizeof(int64_t) * 2 * (R + 1));
    S.pair_ptr.ensure(sizeof(int64_t) * (P + 1));
    S.pin_off.ensure(sizeof(int64_t) * 2 * (R + 1));
    std::memcpy(S.pin_off.p, off.data(), sizeof(int64_t) * 2 * (R + 1));
    FM_HIP_CHECK(hipMemcpyAsync(S.src_off.p, S.pin_off.p, sizeof(int64_t) * 2 * (R + 1), hipMemcpyHostToDevice, st));
    int64_t* pair_ptr = S.pair_ptr.as<int64_t>();
    // the pair table closes with n (pair_ptr[P])
    FM_HIP_CHECK(hipMemcpyAsync(pair_ptr + P, S.src_off.as<int64_t>() + R, sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    // the slot sort's payload: {pair index at this owner, x}; one source numbers its pairs from 0,
    // so the received entries already are that (no copy)
    const uint2* ent2 = reinterpret_cast<const uint2*>(recv_ent);
    if (n > 0) {
      if (R > 1) {
        ctx->sh_ent2.ensure(sizeof(uint2) * n);
        ent2 = ctx->sh_ent2.as<uint2>();
      }
      hipLaunchKernelGGL(k_pair_table, dim3(grid_for(n, kBlock, kShardGrid)), dim3(kBlock), 0, st, reinterpret_cast<const uint2*>(recv_ent),
                         n, S.src_off.as<int64_t>(), S.src_off.as<int64_t>() + (R + 1), R, pair_ptr,
                         R > 1 ? ctx->sh_ent2.as<uint2>() : nullptr);
      FM_HIP_CHECK(hipGetLastError());
    }
    FM_HIP_CHECK(hipEventRecord(S.ready_fwd, st));
    if (n > 0) {
      // the update's grouping: received entries sorted by slot (stable: source rank, then CSR order)
      S.skeys.ensure(sizeof(uint32_t) * n);
      S.sents.ensure(sizeof(uint2) * n);
      const uint32_t* sk = nullptr;
      const uint2* sv = nullptr;
      const uint32_t* keys = reinterpret_cast<const uint32_t*>(recv_slot);
      const int kb = bits_for(std::max<int64_t>(ctx->rows - 1, 1));
      radix_sort_pairs64(ctx->side_sort, keys, ent2, n, kb, st, &sk, &sv, S.skeys.as<uint32_t>(), S.sents.as<uint2>());
    }
    FM_HIP_CHECK(hipEventRecord(S.ready_upd, st));
    ctx->prof_end("owner_prepare", e0, st);
    S.recv_slot = reinterpret_cast<const uint32_t*>(recv_slot);
    S.recv_ent = reinterpret_cast<const uint2*>(recv_ent);
    S.n = n;
    S.P = P;
    S.prepared = true;
    return FM_OK;
  });
}

int fm_shard_owner_forward(fm_ctx* ctx, fm_batch* b, void* partials_out) {
  return guarded(ctx, [&]() -> int {
    require_squared(ctx, "fm_shard_owner_forward");
    shard_owner_partials(ctx, b, partials_out, nullptr);
    return FM_OK;
  });
}

}  // extern "C"

namespace fmhip {

void shard_owner_partials(fm_ctx* ctx, fm_batch* b, void* partials_out, uint32_t* present_out, int chunk,
                          int chunks) {
  ShardBatchState& S = shard_state(ctx, b);
  FM_REQUIRE(S.prepared, "fm_shard_owner_prepare must run on this batch first");
  FM_REQUIRE(S.P == 0 || partials_out, "null buffer");
  const int R = ctx->cfg.shard_count;
  FM_REQUIRE(chunks >= 1 && chunk >= 0 && chunk < chunks && (chunks == 1 || R <= kMaxChunkSources),
             "bad owner-forward chunk");
  hipStream_t st = ctx->stream;
  FM_HIP_CHECK(hipStreamWaitEvent(st, S.ready_fwd, 0));
  if (chunk == 0) S.fwd_e0 = ctx->prof_begin(st);  // the profile spans every chunk
  if (S.P > 0) {
    // partial forward over the pairs, rows of the local table (lazy L1 caught up on read)
    BatchDev view;
    view.n_rows = S.P;
    view.nnz = S.n;
    view.row_ptr.borrow(S.pair_ptr.p, S.pair_ptr.bytes);
    view.col.borrow(S.recv_slot, sizeof(uint32_t) * S.n);
    view.ent.borrow(S.recv_ent, sizeof(uint2) * S.n);
    StepParams p{};
    p.cumE = ctx->cum_host.back();
    int64_t nblk = 0;
    FwdOut xo{};  // the partial pass (partial_out given); only the present counts and the chunk are read
    xo.pcount = present_out;
    if (chunks > 1) {
      xo.ch_off = S.src_off.as<int64_t>() + (R + 1);  // the sources' pair offsets (owner_prepare)
      xo.ch_R = R;
      xo.ch_c = chunk;
      xo.ch_C = chunks;
    }
    launch_forward(ctx->view(), view, ctx->work, p, st, &nblk, reinterpret_cast<float*>(partials_out), &xo,
                   ctx->cfg.wire == FM_WIRE_FP64);
    FM_HIP_CHECK(hipGetLastError());
  }
  if (chunk + 1 == chunks) {
    ctx->prof_end("owner_forward", S.fwd_e0, st);
    S.fwd_e0 = nullptr;
  }
}

void shard_combine_predict(fm_ctx* ctx, fm_batch* b, const void* partials_in, const uint32_t* present_in,
                           double lo, double hi, double* pred_dev) {
  const ReqPlan q = requester_plan(ctx, b, shard_state(ctx, b));
  if (q.B == 0) return;
  FM_REQUIRE(q.Ps == 0 || (partials_in && present_in), "null buffer");
  launch_requester<kReqPredict>(ctx, q, partials_in, present_in, lo, hi, pred_dev);
}

void shard_combine_evaluate(fm_ctx* ctx, fm_batch* b, const void* partials_in, const uint32_t* present_in,
                            double lo, double hi, double* pred_dev, double* rec_dev) {
  const ReqPlan q = requester_plan(ctx, b, shard_state(ctx, b));
  if (q.B == 0) return;
  FM_REQUIRE(q.Ps == 0 || (partials_in && present_in), "null buffer");
  FM_REQUIRE(rec_dev != nullptr, "null buffer");
  hipEvent_t e0 = ctx->prof_begin(ctx->stream);
  ctx->work.eval_part.ensure_slack(sizeof(double) * kEvalRec * kLossPartBlocks);  // the grid's cap: no growth later
  launch_requester<kReqEvaluate>(ctx, q, partials_in, present_in, lo, hi, b->dev.label.as<const double>(), pred_dev,
                                 ctx->work.eval_part.as<double>());
  launch_eval_fold(ctx->work.eval_part.as<double>(), q.blocks, rec_dev, ctx->stream);
  ctx->prof_end("evaluate", e0, ctx->stream);
}

}  // namespace fmhip

extern "C" {

int fm_shard_combine(fm_ctx* ctx, fm_batch* b, const void* partials_in, void* s_send) {
  return guarded(ctx, [&]() -> int {
    require_squared(ctx, "fm_shard_combine");
    ShardBatchState& S = shard_state(ctx, b);
    const ReqPlan q = requester_plan(ctx, b, S);
    FM_REQUIRE(q.Ps == 0 || (partials_in && s_send), "null buffer");
    hipStream_t st = ctx->stream;
    hipEvent_t e0 = ctx->prof_begin(st);
    ctx->work.loss_part.ensure(sizeof(double2) * kLossPartBlocks);  // reserve_work's size: no reallocation later
    float* s_vec = reinterpret_cast<float*>(s_send);
    launch_requester<kReqCombine>(ctx, q, partials_in, b->dev.label.as<double>(), s_vec,
                            wire_scalars<float2>(s_vec, q.Ps, q.kp), ctx->work.loss_part.as<double2>());
    ctx->prof_end("combine", e0, st);
    S.loss_blocks = q.blocks;
    S.combined = true;
    return FM_OK;
  });
}

int fm_shard_owner_update(fm_ctx* ctx, fm_batch* b, const void* s_recv, int32_t t, double step_size,
                          double reg_param, int64_t global_rows) {
  return guarded(ctx, [&]() -> int {
    require_squared(ctx, "fm_shard_owner_update");
    ShardBatchState& S = shard_state(ctx, b);
    FM_REQUIRE(global_rows >= 0, "negative global_rows");
    if (global_rows == 0) return FM_NOTHING_TO_DO;  // SGD.scala:126-128 (every rank skips)
    FM_REQUIRE(t >= 1, "iteration index t must be >= 1");
    FM_REQUIRE(std::isfinite(step_size) && std::isfinite(reg_param), "non-finite step size / regParam");
    FM_REQUIRE(S.prepared && S.combined, "owner_prepare, owner_forward and combine must run on this batch first");
    const int64_t n = S.n;
    FM_REQUIRE(S.P == 0 || s_recv != nullptr, "null buffer");
    hipStream_t st = ctx->stream;
    StepParams p = shard_params(ctx, t, step_size, reg_param, global_rows);
    ctx->ensure_hist(ctx->epoch + 1);
    double* stats = ctx->loss_hist.as<double>() + 3 * (int64_t)ctx->epoch;
    FM_HIP_CHECK(hipStreamWaitEvent(st, S.ready_upd, 0));
    hipEvent_t e0 = ctx->prof_begin(st);
    const float* Srow = reinterpret_cast<const float*>(s_recv);  // [P][kp] S, then [P] {r, yhat}
    const int kp = ctx->kp;
    SegSource src{Srow, kp, wire_scalars<const float2>(Srow, S.P, kp), 1};
    if (s_rec_yl(kp) && S.P > 0) {
      // one record per pair (S and {r, yhat} in one line), as the single-table step's
      const int rec = s_rec_floats(kp);
      ctx->work.S.ensure(sizeof(float) * (size_t)S.P * rec);
      const int64_t nq = S.P * (rec / 4);
      hipLaunchKernelGGL(k_pack_srec, dim3(grid_for(nq, kBlock, kShardGrid)), dim3(kBlock), 0, st, Srow, src.yl, S.P, kp, rec,
                         ctx->work.S.as<float>());
      FM_HIP_CHECK(hipGetLastError());
      src = SegSource{ctx->work.S.as<float>(), rec, reinterpret_cast<const float2*>(ctx->work.S.as<float>() + kp), rec / 2};
    }
    launch_segment_update(ctx->view(), n, src, ctx->work, p, S.skeys.as<uint32_t>(), S.sents.as<uint2>(),
                          S.loss_blocks, stats, st);
    ctx->prof_end("owner_update", e0, st);
    FM_HIP_CHECK(hipEventRecord(S.last_use, st));
    // the iteration's last main-stream read of this rank's batch (its combine read the labels before
    // this): a refill of the batch (fm_batch_from_rows, copy stream) waits for it
    if (b->last_use) FM_HIP_CHECK(hipEventRecord(b->last_use, st));
    ctx->epoch += 1;
    ctx->cum_host.push_back(p.cum_next);
    S.prepared = false;
    S.combined = false;
    S.recv_slot = nullptr;
    S.recv_ent = nullptr;
    return FM_OK;
  });
}

}  // extern "C"

namespace fmhip {

ShardGeometry shard_geometry(int kp) {
  ShardGeometry g{};
  g.pair_tile = kBlock;
  g.route_team = kTeamR;
  g.mask_sweep = kShardGrid * (kBlock / kTeamR);
  g.scan_trip = kBlock;
  g.route_sweep = kShardGrid * kBlock;
  g.route_unroll = kRkU;
  g.table_sweep = kShardGrid * kBlock;
  g.table_unroll = kPtU;
  g.slot_regs = kSlotRegs;
  g.max_r = kMaxR;
  g.combine_team = team_for(kp / 4);
  g.combine_sweep = (int64_t)kLossPartBlocks * (kBlock / g.combine_team);
  g.pack_sweep = s_rec_yl(kp) ? kShardGrid * kBlock / (s_rec_floats(kp) / 4) : 0;
  return g;
}

}  // namespace fmhip
