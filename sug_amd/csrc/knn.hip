// kNN graph over one cloud (replaces knn(), model/model_utils.py:178-185) and the
// reverse neighbour lists used by the EdgeConv backward.
//
// Layout: x [B,N,C] point-major rows (row stride ldx).  One thread owns one query
// point and keeps its K best (score, index) pairs sorted in registers; candidate
// rows are streamed through LDS in tiles of TJ points, read back as wave-wide
// broadcasts (every lane reads the same candidate -> conflict-free).
//
// Roofline: algorithmic bytes 4*C*N + 4*N*k per cloud, FLOPs N^2*(2C+3): compute
// bound for every C; the [B,N,N] matrix of the reference never exists.
#include "common.h"
#include "internal.h"
#include "device_helpers.h"

namespace {

template <int K>
__device__ __forceinline__ void topk_insert_desc(float (&v)[K], int (&id)[K], float s, int j) {
  // precondition s > v[K-1]; strict compares keep earlier (lower) j first among ties
#pragma unroll
  for (int t = K - 1; t > 0; --t) {
    const bool up = s > v[t - 1];
    const bool here = s > v[t];
    const float nv = up ? v[t - 1] : (here ? s : v[t]);
    const int ni = up ? id[t - 1] : (here ? j : id[t]);
    v[t] = nv;
    id[t] = ni;
  }
  if (s > v[0]) {
    v[0] = s;
    id[0] = j;
  }
}

// row stride of the candidate tile in LDS: +4 keeps 16-B alignment for the
// broadcast float4 reads and de-conflicts the per-candidate norm pass.
template <int C>
struct TileStride { static constexpr int value = (C % 4 == 0) ? C + 4 : C; };

template <int C, int K, int BLOCK, int TJ>
__global__ __launch_bounds__(BLOCK) void knn_self_kernel(const float* __restrict__ x, int64_t ldx,
                                                         int N, int k, int32_t* __restrict__ idx) {
  constexpr int CS = TileStride<C>::value;
  __shared__ __attribute__((aligned(16))) float s_x[TJ * CS];
  __shared__ float s_n[TJ];
  const int b = blockIdx.y;
  const float* xb = x + (int64_t)b * N * ldx;
  const int q = blockIdx.x * BLOCK + threadIdx.x;
  const int qc = q < N ? q : N - 1;

  float xi[C];
#pragma unroll
  for (int c = 0; c < C; ++c) xi[c] = xb[(int64_t)qc * ldx + c];
  float ni = __fmul_rn(xi[0], xi[0]);
#pragma unroll
  for (int c = 1; c < C; ++c) ni = __fadd_rn(ni, __fmul_rn(xi[c], xi[c]));

  float v[K];
  int id[K];
#pragma unroll
  for (int t = 0; t < K; ++t) {
    v[t] = -INFINITY;
    id[t] = 0;
  }

  for (int j0 = 0; j0 < N; j0 += TJ) {
    __syncthreads();
    for (int e = threadIdx.x; e < TJ * C; e += BLOCK) {
      const int r = e / C, c = e - r * C;
      const int j = j0 + r;
      s_x[r * CS + c] = j < N ? xb[(int64_t)j * ldx + c] : 0.0f;
    }
    __syncthreads();
    for (int r = threadIdx.x; r < TJ; r += BLOCK) {
      const float* xr = s_x + r * CS;
      float nj = __fmul_rn(xr[0], xr[0]);
#pragma unroll 8
      for (int c = 1; c < C; ++c) nj = __fadd_rn(nj, __fmul_rn(xr[c], xr[c]));
      s_n[r] = nj;
    }
    __syncthreads();
    const int rmax = (N - j0) < TJ ? (N - j0) : TJ;
    for (int r = 0; r < rmax; ++r) {
      const float* xr = s_x + r * CS;
      float acc;
      if constexpr (C % 4 == 0) {
        const float4* xr4 = reinterpret_cast<const float4*>(xr);
        float4 t = xr4[0];
        acc = __fmul_rn(xi[0], t.x);
        acc = fmaf(xi[1], t.y, acc);
        acc = fmaf(xi[2], t.z, acc);
        acc = fmaf(xi[3], t.w, acc);
#pragma unroll
        for (int c4 = 1; c4 < C / 4; ++c4) {
          t = xr4[c4];
          acc = fmaf(xi[4 * c4 + 0], t.x, acc);
          acc = fmaf(xi[4 * c4 + 1], t.y, acc);
          acc = fmaf(xi[4 * c4 + 2], t.z, acc);
          acc = fmaf(xi[4 * c4 + 3], t.w, acc);
        }
      } else {
        acc = __fmul_rn(xi[0], xr[0]);
#pragma unroll
        for (int c = 1; c < C; ++c) acc = fmaf(xi[c], xr[c], acc);
      }
      // pairwise_distance = -xx - inner - xx^T, inner = -2*dot (model_utils.py:179-181)
      const float s = __fsub_rn(__fsub_rn(-s_n[r], __fmul_rn(-2.0f, acc)), ni);
      if (s > v[K - 1]) topk_insert_desc<K>(v, id, s, j0 + r);
    }
  }
  if (q < N) {
    int32_t* o = idx + ((int64_t)b * N + q) * k;
#pragma unroll
    for (int t = 0; t < K; ++t)
      if (t < k) o[t] = id[t];
  }
}

// Any C: the query row stays in global memory (L1-resident), candidates in LDS.
template <int K, int BLOCK, int TJ>
__global__ __launch_bounds__(BLOCK) void knn_self_generic_kernel(const float* __restrict__ x,
                                                                 int64_t ldx, int N, int C, int k,
                                                                 int32_t* __restrict__ idx) {
  extern __shared__ float s_dyn[];  // TJ*C candidate tile
  const int b = blockIdx.y;
  const float* xb = x + (int64_t)b * N * ldx;
  const int q = blockIdx.x * BLOCK + threadIdx.x;
  const int qc = q < N ? q : N - 1;
  const float* xq = xb + (int64_t)qc * ldx;
  float ni = __fmul_rn(xq[0], xq[0]);
  for (int c = 1; c < C; ++c) ni = __fadd_rn(ni, __fmul_rn(xq[c], xq[c]));
  float v[K];
  int id[K];
#pragma unroll
  for (int t = 0; t < K; ++t) {
    v[t] = -INFINITY;
    id[t] = 0;
  }
  for (int j0 = 0; j0 < N; j0 += TJ) {
    __syncthreads();
    for (int e = threadIdx.x; e < TJ * C; e += BLOCK) {
      const int r = e / C, c = e - r * C;
      const int j = j0 + r;
      s_dyn[e] = j < N ? xb[(int64_t)j * ldx + c] : 0.0f;
    }
    __syncthreads();
    const int rmax = (N - j0) < TJ ? (N - j0) : TJ;
    for (int r = 0; r < rmax; ++r) {
      const float* xr = s_dyn + r * C;
      float acc = __fmul_rn(xq[0], xr[0]);
      float nj = __fmul_rn(xr[0], xr[0]);
      for (int c = 1; c < C; ++c) {
        acc = fmaf(xq[c], xr[c], acc);
        nj = __fadd_rn(nj, __fmul_rn(xr[c], xr[c]));
      }
      const float s = __fsub_rn(__fsub_rn(-nj, __fmul_rn(-2.0f, acc)), ni);
      if (s > v[K - 1]) topk_insert_desc<K>(v, id, s, j0 + r);
    }
  }
  if (q < N) {
    int32_t* o = idx + ((int64_t)b * N + q) * k;
#pragma unroll
    for (int t = 0; t < K; ++t)
      if (t < k) o[t] = id[t];
  }
}

template <int C, int K>
int launch_knn(const float* x, int64_t ldx, int B, int N, int k, int32_t* idx, hipStream_t st) {
  // one wave per block keeps >= 2 blocks per CU at B*N = 32k queries
  constexpr int BLOCK = 64;
  constexpr int TJ = (C >= 64) ? 32 : 128;
  dim3 grid(sug_divup(N, BLOCK), B);
  hipLaunchKernelGGL((knn_self_kernel<C, K, BLOCK, TJ>), grid, dim3(BLOCK), 0, st, x, ldx, N, k, idx);
  SUG_LAUNCH_CHECK("sug_knn");
  return SUG_OK;
}

template <int K>
int dispatch_knn_c(const float* x, int64_t ldx, int B, int N, int C, int k, int32_t* idx,
                   hipStream_t st) {
  switch (C) {
    case 3: return launch_knn<3, K>(x, ldx, B, N, k, idx, st);
    case 64: return launch_knn<64, K>(x, ldx, B, N, k, idx, st);
    case 128: return launch_knn<128, K>(x, ldx, B, N, k, idx, st);
    default: {
      constexpr int BLOCK = 64;
      int TJ = 64;
      while (TJ > 1 && (size_t)TJ * C * sizeof(float) > 48 * 1024) TJ >>= 1;
      SUG_REQUIRE((size_t)TJ * C * sizeof(float) <= 48 * 1024, "sug_knn: C=%d too large", C);
      dim3 grid(sug_divup(N, BLOCK), B);
      // TJ is a template constant of the kernel only through its loop bound: use 64/32/16/...
      size_t sh = (size_t)TJ * C * sizeof(float);
      if (TJ == 64)
        hipLaunchKernelGGL((knn_self_generic_kernel<K, BLOCK, 64>), grid, dim3(BLOCK), sh, st, x, ldx, N, C, k, idx);
      else if (TJ == 32)
        hipLaunchKernelGGL((knn_self_generic_kernel<K, BLOCK, 32>), grid, dim3(BLOCK), sh, st, x, ldx, N, C, k, idx);
      else if (TJ == 16)
        hipLaunchKernelGGL((knn_self_generic_kernel<K, BLOCK, 16>), grid, dim3(BLOCK), sh, st, x, ldx, N, C, k, idx);
      else
        hipLaunchKernelGGL((knn_self_generic_kernel<K, BLOCK, 8>), grid, dim3(BLOCK), (size_t)8 * C * sizeof(float), st, x, ldx, N, C, k, idx);
      SUG_LAUNCH_CHECK("sug_knn(generic)");
      return SUG_OK;
    }
  }
}

// ---- reverse lists ---------------------------------------------------------
// A stable counting placement, no atomics and no per-list sort: every entry goes straight to its final place.
// A workgroup owns the destinations [lo, hi) of one cloud (RS ranges per cloud, so that 64 clouds fill the chip):
//   1. it loads the cloud's E entries ONCE into registers (wave w holds the contiguous span of U*64 entries behind
//      w*U*64, U = ceil(E / 1024), every load in flight before the first use);
//   2. it compacts the entries that point into its range into LDS IN ENTRY ORDER (ballot + prefix popcount per 64
//      entries, wave totals scanned across the waves), packed as (destination - lo) << 16 | entry; the entries that
//      point below the range are counted the same way: the range's base offset in the cloud's entry array;
//   3. LSD radix sort of the compacted array by the local destination, two bits a pass: a thread owns a contiguous
//      run of R = ceil(count / 1024) items, which it keeps in registers between the read and the scatter (the sort is
//      in place), and a private 4-bin histogram in one 64-bit register (16-bit fields, which cannot carry: no bin of
//      the workgroup holds 65536 items); the (digit-major, thread-minor) scan is a DPP wave scan of that register and,
//      in every wave, a scan of the 4 x 16 wave totals.  The scanned register is the thread's four running write
//      positions.  Stable, so the entries of a destination stay ascending;
//   4. rev_off by a binary search of every destination in the sorted array, rev_ent copied out coalesced.
// The work depends on the number of entries in the range (R), not on how they are spread over its destinations.
// LDS: 32 ints of scratch + E packed items (a range may hold every entry), always within what
// sug_reverse_lists_lds_bytes reports; E < 65536 and the range < 32768 destinations follow from its 160 KB bound.
constexpr int REV_BLOCK = 1024;
constexpr int REV_NW = REV_BLOCK / 64;
static_assert(REV_NW == 16, "4 bins x 16 waves: the 64 totals a wave scans, 8 bytes a wave in the 32 scratch ints");

template <int UMAX>
__global__ __launch_bounds__(REV_BLOCK) void reverse_lists_kernel(const int32_t* __restrict__ idx, int N, int E, int RS,
                                                                  int32_t* __restrict__ rev_off,
                                                                  int32_t* __restrict__ rev_ent) {
  // E entries per cloud (N*k for a kNN graph, S*nsample for ball-query lists), destinations in [0, N)
  extern __shared__ int s_i[];                  // scratch[32] | item[E]
  int* scr = s_i;
  unsigned* tot = reinterpret_cast<unsigned*>(s_i);                    // [REV_NW] x 4 digit totals of 16 bits
  const unsigned short* tot16 = reinterpret_cast<const unsigned short*>(s_i);
  unsigned* item = reinterpret_cast<unsigned*>(s_i + 2 * REV_NW);
  const int Nr = (N + RS - 1) / RS;
  // workgroups x and x + 8 are observed to share an L2 (speed only, nothing depends on it): the RS workgroups of a cloud,
  // which all read its whole entry array, are made neighbours in that sense when the grid divides by 8
  const int G = gridDim.x;
  const int wg = (G % 8 == 0) ? (int)(blockIdx.x % 8) * (G / 8) + (int)(blockIdx.x / 8) : (int)blockIdx.x;
  const int b = wg / RS, r = wg % RS;
  const int lo = min(r * Nr, N), hi = min(lo + Nr, N);
  const int nr = hi - lo;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int32_t* ib = idx + (int64_t)b * E;
  int32_t* off = rev_off + (int64_t)b * (N + 1);
  int32_t* gent = rev_ent + (int64_t)b * E;

  const int U = (E + REV_BLOCK - 1) / REV_BLOCK;                       // <= UMAX (the launcher's choice)
  const int e0 = wave * U * 64 + lane;
  int mv[UMAX];
#pragma unroll
  for (int u = 0; u < UMAX; ++u) {
    const int e = e0 + u * 64;
    mv[u] = (u < U && e < E) ? ib[e] : -1;
  }
  // counts of this wave: entries into the range, valid entries below it (ballots: wave-uniform, integer, order-free)
  int mine = 0, below = 0;
#pragma unroll
  for (int u = 0; u < UMAX; ++u) {
    if (u < U) {
      const unsigned m = (unsigned)mv[u];
      mine += __popcll(__ballot(m - (unsigned)lo < (unsigned)nr));
      below += __popcll(__ballot(m < (unsigned)lo));
    }
  }
  if (lane == 0) {
    scr[wave] = mine;
    scr[REV_NW + wave] = below;
  }
  __syncthreads();
  // row 0 of every wave scans the 16 counts, row 1 the 16 counts below the range
  const unsigned sc = rev_row_scan(lane < 2 * REV_NW ? (unsigned)scr[lane] : 0u);
  const int count = __builtin_amdgcn_readlane((int)sc, REV_NW - 1);
  const int base = __builtin_amdgcn_readlane((int)sc, 2 * REV_NW - 1);
  int run = wave > 0 ? __builtin_amdgcn_readlane((int)sc, max(wave - 1, 0)) : 0;
#pragma unroll
  for (int u = 0; u < UMAX; ++u) {
    if (u < U) {
      const unsigned key = (unsigned)mv[u] - (unsigned)lo;
      const bool in = key < (unsigned)nr;
      const unsigned long long bal = __ballot(in);
      const unsigned at = __builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, (unsigned)run));
      if (in) item[at] = (key << 16) | (unsigned)(e0 + u * 64);
      run += __popcll(bal);
    }
  }
  __syncthreads();                              // the scratch is the sort's behind this barrier

  const int R = (count + REV_BLOCK - 1) / REV_BLOCK;                   // <= U
  const int p0 = threadIdx.x * R;
  const int own = min(max(count - p0, 0), R);                          // items of this thread's run
  int keybits = 0;
  while ((1 << keybits) < nr) ++keybits;
  for (int sh = 16; sh < 16 + keybits; sh += 2) {
    unsigned it[UMAX];
    unsigned long long h = 0;                   // bins 0 .. 3, 16 bits each
#pragma unroll
    for (int u = 0; u < UMAX; ++u) {
      if (u < R) {                              // uniform over the workgroup
        if (u < own) {
          it[u] = item[p0 + u];
          h += 1ull << ((it[u] >> (sh - 4)) & 0x30u);
        }
      }
    }
    // inclusive over the wave's lanes (a wave holds at most 64 * UMAX items)
    const unsigned ilo = rev_wave_scan((unsigned)h), ihi = rev_wave_scan((unsigned)(h >> 32));
    if (lane == 63) {
      tot[2 * wave] = ilo;
      tot[2 * wave + 1] = ihi;
    }
    __syncthreads();                            // every item of this pass is in registers behind this barrier
    // every wave scans the 64 totals for itself, digit-major: lane d*16 + w holds bin d of wave w
    const unsigned v = tot16[(lane & 15) * 4 + (lane >> 4)];
    const unsigned x = rev_wave_scan(v) - v;
    const unsigned s0 = (unsigned)__builtin_amdgcn_readlane((int)x, wave);
    const unsigned s1 = (unsigned)__builtin_amdgcn_readlane((int)x, 16 + wave);
    const unsigned s2 = (unsigned)__builtin_amdgcn_readlane((int)x, 32 + wave);
    const unsigned s3 = (unsigned)__builtin_amdgcn_readlane((int)x, 48 + wave);
    // the thread's four write positions: bins before + waves before + lanes before, field by field (all <= count)
    const unsigned clo = (s0 | (s1 << 16)) + (ilo - (unsigned)h), chi = (s2 | (s3 << 16)) + (ihi - (unsigned)(h >> 32));
    unsigned long long cur = ((unsigned long long)chi << 32) | clo;
#pragma unroll
    for (int u = 0; u < UMAX; ++u) {
      if (u < R) {
        if (u < own) {
          const unsigned sft = (it[u] >> (sh - 4)) & 0x30u;
          item[(unsigned)(cur >> sft) & 0xffffu] = it[u];
          cur += 1ull << sft;
        }
      }
    }
    __syncthreads();
  }

  for (int p = threadIdx.x; p < count; p += REV_BLOCK) gent[base + p] = (int)(item[p] & 0xffffu);
  // rev_off[lo + i] = base + the first position whose destination is >= i (behind the stores above, which drain meanwhile)
  for (int i = threadIdx.x; i < nr; i += REV_BLOCK) {
    int a = 0, n = count;
    while (n > 0) {
      const int half = n >> 1;
      if ((int)(item[a + half] >> 16) < i) {
        a += half + 1;
        n -= half + 1;
      } else {
        n = half;
      }
    }
    off[lo + i] = base + a;
  }
  if (r == RS - 1 && threadIdx.x == 0) off[N] = base + count;
}

template <int UMAX>
int reverse_lists_launch(const int32_t* idx, int B, int E, int N, int RS, int32_t* rev_off, int32_t* rev_ent,
                         hipStream_t st) {
  static SugLdsOptIn note;
  if (int rc = sug_allow_dynamic_lds(note, &reverse_lists_kernel<UMAX>, 160 * 1024, "sug_reverse_lists")) return rc;
  const size_t sh = (size_t)(2 * REV_NW + E) * sizeof(int);
  hipLaunchKernelGGL((reverse_lists_kernel<UMAX>), dim3(B * RS), dim3(REV_BLOCK), sh, st, idx, N, E, RS, rev_off,
                     rev_ent);
  SUG_LAUNCH_CHECK("sug_reverse_lists");
  return SUG_OK;
}

}  // namespace

extern "C" int sug_knn(const float* x, int64_t ldx, int B, int N, int C, int k, int32_t* idx,
                       void* stream) {
  SUG_REQUIRE(x && idx, "sug_knn: null pointer");
  SUG_REQUIRE(B > 0 && N > 0 && C > 0, "sug_knn: bad shape B=%d N=%d C=%d", B, N, C);
  SUG_REQUIRE(k >= 1 && k <= 32 && k <= N, "sug_knn: need 1 <= k <= min(32,N), got k=%d N=%d", k, N);
  SUG_REQUIRE(ldx >= C, "sug_knn: ldx=%lld < C=%d", (long long)ldx, C);
  SUG_REQUIRE(B <= 65535, "sug_knn: B=%d exceeds grid.y", B);
  hipStream_t st = (hipStream_t)stream;
  if (sug_knn_pc_supported(x, ldx, C, k)) return sug_knn_pc(x, ldx, B, N, C, k, idx, st);
  if (k <= 16) return dispatch_knn_c<16>(x, ldx, B, N, C, k, idx, st);
  if (k <= 20) return dispatch_knn_c<20>(x, ldx, B, N, C, k, idx, st);
  return dispatch_knn_c<32>(x, ldx, B, N, C, k, idx, st);
}

// LDS bytes that decide whether the reverse-list build takes B clouds of E entries into N destinations (and its destination
// ranges per cloud): callers that need to know beforehand whether sug_reverse_lists will take the shape compare this with
// 160 KB.  The formula is that of the build the list-based backwards were shaped around (two counters per destination of a
// range); it is kept as it is because it chooses between a list-based backward and its fallback, which sum in different
// orders.  reverse_lists_kernel needs no more than it for any shape (32 + E ints).
size_t sug_reverse_lists_lds_bytes(int B, int E, int N, int* ranges) {
  int RS = 1;                                    // destination ranges per cloud: >= 256 workgroups when B allows
  while (RS < 8 && B * RS < 256 && N / (RS * 2) >= 64) RS *= 2;
  const int Nr = (N + RS - 1) / RS;
  if (ranges) *ranges = RS;
  return (size_t)(2 * Nr + 2 * (1024 / 64) + (size_t)E) * sizeof(int);
}

// reverse lists of B clouds with E index entries each, destinations in [0, N); the lists always come out ascending
// (sorted = 0 only says that the consumer would not need it: the stable placement has no cheaper unordered form)
int sug_reverse_lists(const int32_t* idx, int B, int E, int N, int sorted, int32_t* rev_off, int32_t* rev_ent,
                      hipStream_t st) {
  (void)sorted;
  SUG_REQUIRE(idx && rev_off && rev_ent, "sug_reverse_lists: null pointer");
  SUG_REQUIRE(B > 0 && N > 0 && E > 0, "sug_reverse_lists: bad shape");
  int RS = 0;
  const size_t sh = sug_reverse_lists_lds_bytes(B, E, N, &RS);
  SUG_REQUIRE(sh <= 160 * 1024, "sug_reverse_lists: %d entries per cloud are too many for the LDS-resident build", E);
  const int U = sug_divup(E, REV_BLOCK);         // entries a thread holds in registers: <= 40 by the bound above
  if (U <= 8) return reverse_lists_launch<8>(idx, B, E, N, RS, rev_off, rev_ent, st);
  if (U <= 20) return reverse_lists_launch<20>(idx, B, E, N, RS, rev_off, rev_ent, st);
  SUG_REQUIRE(U <= 40, "sug_reverse_lists: %d entries per cloud are too many for the LDS-resident build", E);
  return reverse_lists_launch<40>(idx, B, E, N, RS, rev_off, rev_ent, st);
}

extern "C" int sug_reverse_lists_build(const int32_t* idx, int B, int E, int N, int sorted, int32_t* rev_off,
                                       int32_t* rev_ent, void* stream) {
  return sug_reverse_lists(idx, B, E, N, sorted, rev_off, rev_ent, (hipStream_t)stream);
}

extern "C" int sug_knn_reverse(const int32_t* idx, int B, int N, int k, int32_t* rev_off,
                               int32_t* rev_ent, void* stream) {
  SUG_REQUIRE(B > 0 && N > 0 && k > 0, "sug_knn_reverse: bad shape");
  const int64_t E = (int64_t)N * k;
  // the LDS-resident build where it takes the shape (what it launches does not change), the tiled build behind it
  if (E <= 40 * REV_BLOCK && sug_reverse_lists_lds_bytes(B, (int)E, N, nullptr) <= 160 * 1024)
    return sug_reverse_lists(idx, B, (int)E, N, 1, rev_off, rev_ent, (hipStream_t)stream);
  SUG_REQUIRE(E <= SUG_REV_TILED_MAX_ENTRIES, "sug_knn_reverse: N * k = %lld entries per cloud exceed SUG_REV_TILED_MAX_ENTRIES=%d",
              (long long)E, SUG_REV_TILED_MAX_ENTRIES);
  return sug_reverse_lists_tiled(idx, B, (int)E, N, 0, rev_off, rev_ent, stream);
}
