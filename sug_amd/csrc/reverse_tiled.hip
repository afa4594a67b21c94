// Reverse neighbour lists for clouds beyond the LDS-resident build of knn.hip (reverse_lists_kernel): the same stable
// counting placement with the cloud streamed through LDS in tiles.  sug_knn_reverse (knn.hip) hands over the shapes its
// own build refuses; sug_reverse_lists_tiled takes any shape within SUG_REV_TILED_MAX_DEST / _MAX_ENTRIES.
#include "common.h"
#include "device_helpers.h"

namespace {

constexpr int REV_BLOCK = 1024;
constexpr int REV_NW = REV_BLOCK / 64;
static_assert(REV_NW == 16, "4 bins x 16 waves: the 64 totals a wave scans, 8 bytes a wave in the 32 scratch ints");

// ---- tiled reverse lists ---------------------------------------------------
// The same placement for clouds of any size: reverse_lists_kernel is its one-tile case.  A workgroup owns the destinations
// [lo, hi) of one cloud and streams the cloud's E entries in tiles of T = 1024 * U entries, twice:
//   pass 1  per tile, the entries in registers as in knn.hip (wave w holds a contiguous span of the tile): the valid
//           entries below the range are counted with ballots (the range's base in rev_ent), the entries of every destination of the range with integer LDS adds (exact, order-free;
//           a wave whose entries into the range all name one destination adds once).  No barrier between tiles;
//   scan    of the counts (a thread owns a contiguous chunk, DPP wave scan, the 16 wave totals scanned in every wave): rev_off,
//           and in LDS one running CURSOR per destination, the place of its next entry in rev_ent;
//   pass 2  per tile: compacted in entry order as (destination - lo) << 16 | entry WITHIN THE TILE, sorted stably by the
//           two-bit radix passes of knn.hip, then every run of equal destinations goes to its cursor with plain stores: the run's
//           first item p0 turns the cursor into (cursor - p0), every item p stores the tile's base + its entry at
//           cursor + p, the run's last item p1 leaves cursor + p1 + 1 behind: advanced by the run length.  Tiles come in
//           entry order and the sort is stable, so a destination's entries stay ascending across tiles.
// Nothing but idx is read from global memory and nothing is added there: no workspace, no atomics on global memory.
// LDS: 32 ints of scratch + T items + one cursor per destination of the range (<= REVT_MAX_RANGE by the range count).
constexpr int REVT_MAX_RANGE = 8192;
static_assert(4 * (2 * REV_NW + SUG_REV_TILED_MAX_TILE + REVT_MAX_RANGE) <= 160 * 1024, "scratch, tile and cursors in LDS");
static_assert(SUG_REV_TILED_MAX_TILE % REV_BLOCK == 0 && SUG_REV_TILED_MAX_TILE < 65536, "16-bit entry and histogram fields");

// destination ranges per cloud: those of the LDS build, doubled until a range's cursors fit beside the largest tile
int revt_ranges(int B, int N) {
  int RS = 1;
  while (RS < 8 && (int64_t)B * RS < 256 && N / (RS * 2) >= 64) RS *= 2;
  while (sug_divup(N, RS) > REVT_MAX_RANGE) RS *= 2;
  return RS;
}

// in-place stable LSD radix sort of item[0, count) by the bits [16, 16 + keybits), two a pass: reverse_lists_kernel's step 3
// (count <= 1024 * UMAX < 65536); every thread calls it, the items are sorted behind its last barrier
template <int UMAX>
__device__ __forceinline__ void revt_sort(unsigned* item, unsigned* tot, int count, int keybits, int lane, int wave) {
  const unsigned short* tot16 = reinterpret_cast<const unsigned short*>(tot);
  const int R = (count + REV_BLOCK - 1) / REV_BLOCK;
  const int p0 = threadIdx.x * R;
  const int own = min(max(count - p0, 0), R);
  for (int sh = 16; sh < 16 + keybits; sh += 2) {
    unsigned it[UMAX];
    unsigned long long h = 0;
#pragma unroll
    for (int u = 0; u < UMAX; ++u) {
      if (u < R) {
        if (u < own) {
          it[u] = item[p0 + u];
          h += 1ull << ((it[u] >> (sh - 4)) & 0x30u);
        }
      }
    }
    const unsigned ilo = rev_wave_scan((unsigned)h), ihi = rev_wave_scan((unsigned)(h >> 32));
    if (lane == 63) {
      tot[2 * wave] = ilo;
      tot[2 * wave + 1] = ihi;
    }
    __syncthreads();
    const unsigned v = tot16[(lane & 15) * 4 + (lane >> 4)];
    const unsigned x = rev_wave_scan(v) - v;
    const unsigned s0 = (unsigned)__builtin_amdgcn_readlane((int)x, wave);
    const unsigned s1 = (unsigned)__builtin_amdgcn_readlane((int)x, 16 + wave);
    const unsigned s2 = (unsigned)__builtin_amdgcn_readlane((int)x, 32 + wave);
    const unsigned s3 = (unsigned)__builtin_amdgcn_readlane((int)x, 48 + wave);
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
}

template <int UMAX>
__global__ __launch_bounds__(REV_BLOCK) void reverse_lists_tiled_kernel(const int32_t* __restrict__ idx, int N, int E, int RS,
                                                                        int T, int32_t* __restrict__ rev_off,
                                                                        int32_t* __restrict__ rev_ent) {
  extern __shared__ int s_i[];                  // scratch[32] | item[T] | cursor[Nr]
  int* scr = s_i;
  unsigned* item = reinterpret_cast<unsigned*>(s_i + 2 * REV_NW);
  int* cur = s_i + 2 * REV_NW + T;
  const int Nr = (N + RS - 1) / RS;
  const int G = gridDim.x;                      // the workgroups of a cloud share an L2 where the grid allows (as in knn.hip)
  const int wg = (G % 8 == 0) ? (int)(blockIdx.x % 8) * (G / 8) + (int)(blockIdx.x / 8) : (int)blockIdx.x;
  const int b = wg / RS, r = wg % RS;
  const int lo = min(r * Nr, N), hi = min(lo + Nr, N);
  const int nr = hi - lo;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int32_t* ib = idx + (int64_t)b * E;
  int32_t* off = rev_off + (int64_t)b * (N + 1);
  int32_t* gent = rev_ent + (int64_t)b * E;
  const int U = T / REV_BLOCK;                  // <= UMAX (the launcher's choice)
  const int e0 = wave * U * 64 + lane;          // within a tile
  const int tiles = (E + T - 1) / T;

  for (int i = threadIdx.x; i < nr; i += REV_BLOCK) cur[i] = 0;
  __syncthreads();

  // pass 1: the counts
  int below = 0;
  for (int t = 0; t < tiles; ++t) {
    const int tb = t * T;
    int mv[UMAX];
#pragma unroll
    for (int u = 0; u < UMAX; ++u) {
      const int e = tb + e0 + u * 64;
      mv[u] = (u < U && e < E) ? ib[e] : -1;
    }
#pragma unroll
    for (int u = 0; u < UMAX; ++u) {
      if (u < U) {
        const unsigned m = (unsigned)mv[u];
        const unsigned key = m - (unsigned)lo;
        const bool in = key < (unsigned)nr;
        below += __popcll(__ballot(m < (unsigned)lo));
        const unsigned long long bal = __ballot(in);
        if (bal != 0) {                         // wave-uniform
          const int first = __builtin_amdgcn_readfirstlane(__builtin_ctzll(bal));
          const unsigned k0 = (unsigned)__builtin_amdgcn_readlane((int)key, first);
          if (__ballot(in && key == k0) == bal) {
            if (lane == first) atomicAdd(&cur[k0], __popcll(bal));
          } else if (in) {
            atomicAdd(&cur[key], 1);
          }
        }
      }
    }
  }
  __syncthreads();

  // scan: cursor[i] = rev_off[lo + i] = base + the counts before i
  const int C = (nr + REV_BLOCK - 1) / REV_BLOCK;
  const int i0 = threadIdx.x * C;
  int sum = 0;
  for (int u = 0; u < C; ++u)
    if (i0 + u < nr) sum += cur[i0 + u];
  const unsigned incl = rev_wave_scan((unsigned)sum);
  if (lane == 0) scr[wave] = below;
  if (lane == 63) scr[REV_NW + wave] = (int)incl;
  __syncthreads();
  // row 0 of every wave scans the 16 counts below the range, row 1 the 16 wave totals
  const unsigned sc = rev_row_scan(lane < 2 * REV_NW ? (unsigned)scr[lane] : 0u);
  const int base = __builtin_amdgcn_readlane((int)sc, REV_NW - 1);
  const int count = __builtin_amdgcn_readlane((int)sc, 2 * REV_NW - 1);
  const int before = wave > 0 ? __builtin_amdgcn_readlane((int)sc, REV_NW + max(wave - 1, 0)) : 0;
  {
    int pos = base + before + (int)incl - sum;
    for (int u = 0; u < C; ++u) {
      if (i0 + u < nr) {
        const int c = cur[i0 + u];
        cur[i0 + u] = pos;
        off[lo + i0 + u] = pos;
        pos += c;
      }
    }
  }
  if (r == RS - 1 && threadIdx.x == 0) off[N] = base + count;
  __syncthreads();                              // the cursors stand, the scratch is free
  if (count == 0) return;                       // uniform over the workgroup

  int keybits = 0;
  while ((1 << keybits) < nr) ++keybits;
  // pass 2: the placement
  for (int t = 0; t < tiles; ++t) {
    const int tb = t * T;
    int mv[UMAX];
#pragma unroll
    for (int u = 0; u < UMAX; ++u) {
      const int e = tb + e0 + u * 64;
      mv[u] = (u < U && e < E) ? ib[e] : -1;
    }
    int mine = 0;
#pragma unroll
    for (int u = 0; u < UMAX; ++u)
      if (u < U) mine += __popcll(__ballot((unsigned)mv[u] - (unsigned)lo < (unsigned)nr));
    if (lane == 0) scr[wave] = mine;
    __syncthreads();                            // also: the previous tile's items and cursors are done with
    const unsigned ws = rev_row_scan(lane < REV_NW ? (unsigned)scr[lane] : 0u);
    const int tcount = __builtin_amdgcn_readlane((int)ws, REV_NW - 1);
    int run = wave > 0 ? __builtin_amdgcn_readlane((int)ws, max(wave - 1, 0)) : 0;
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
    __syncthreads();                            // the scratch is the sort's behind this barrier
    if (tcount == 0) continue;                  // uniform: a tile with no entry of this range
    revt_sort<UMAX>(item, reinterpret_cast<unsigned*>(scr), tcount, keybits, lane, wave);
    for (int p = threadIdx.x; p < tcount; p += REV_BLOCK) {
      const unsigned key = item[p] >> 16;
      if (p == 0 || (item[p - 1] >> 16) != key) cur[key] -= p;
    }
    __syncthreads();
    for (int p = threadIdx.x; p < tcount; p += REV_BLOCK) {
      const unsigned v = item[p];
      gent[cur[v >> 16] + p] = tb + (int)(v & 0xffffu);
    }
    __syncthreads();
    for (int p = threadIdx.x; p < tcount; p += REV_BLOCK) {
      const unsigned key = item[p] >> 16;
      if (p == tcount - 1 || (item[p + 1] >> 16) != key) cur[key] += p + 1;
    }
  }
}

template <int UMAX>
int reverse_lists_tiled_launch(const int32_t* idx, int B, int E, int N, int RS, int T, int32_t* rev_off, int32_t* rev_ent,
                               hipStream_t st) {
  static SugLdsOptIn note;
  if (int rc = sug_allow_dynamic_lds(note, &reverse_lists_tiled_kernel<UMAX>, 160 * 1024, "sug_reverse_lists_tiled")) return rc;
  const size_t sh = (size_t)(2 * REV_NW + T + sug_divup(N, RS)) * sizeof(int);
  hipLaunchKernelGGL((reverse_lists_tiled_kernel<UMAX>), dim3(B * RS), dim3(REV_BLOCK), sh, st, idx, N, E, RS, T, rev_off,
                     rev_ent);
  SUG_LAUNCH_CHECK("sug_reverse_lists_tiled");
  return SUG_OK;
}

}  // namespace

extern "C" int sug_reverse_lists_tiled_supported(int B, int E, int N) {
  return (B > 0 && E > 0 && N > 0 && N <= SUG_REV_TILED_MAX_DEST && E <= SUG_REV_TILED_MAX_ENTRIES &&
          (int64_t)B * revt_ranges(B, N) <= 0x7fffffffll) ? 1 : 0;
}

extern "C" int sug_reverse_lists_tiled(const int32_t* idx, int B, int E, int N, int tile, int32_t* rev_off,
                                       int32_t* rev_ent, void* stream) {
  SUG_REQUIRE(idx && rev_off && rev_ent, "sug_reverse_lists_tiled: null pointer");
  SUG_REQUIRE(B > 0 && N > 0 && E > 0, "sug_reverse_lists_tiled: bad shape B=%d E=%d N=%d", B, E, N);
  SUG_REQUIRE(N <= SUG_REV_TILED_MAX_DEST, "sug_reverse_lists_tiled: N=%d destinations exceed SUG_REV_TILED_MAX_DEST=%d", N,
              SUG_REV_TILED_MAX_DEST);
  SUG_REQUIRE(E <= SUG_REV_TILED_MAX_ENTRIES, "sug_reverse_lists_tiled: E=%d entries per cloud exceed SUG_REV_TILED_MAX_ENTRIES=%d",
              E, SUG_REV_TILED_MAX_ENTRIES);
  SUG_REQUIRE(tile == 0 || (tile % REV_BLOCK == 0 && tile >= REV_BLOCK && tile <= SUG_REV_TILED_MAX_TILE),
              "sug_reverse_lists_tiled: tile=%d is neither 0 nor a multiple of %d in [%d, SUG_REV_TILED_MAX_TILE=%d]", tile,
              REV_BLOCK, REV_BLOCK, SUG_REV_TILED_MAX_TILE);
  const int RS = revt_ranges(B, N);
  SUG_REQUIRE((int64_t)B * RS <= 0x7fffffffll, "sug_reverse_lists_tiled: B=%d clouds exceed the grid", B);
  // the library's choice: the whole cloud when it fits the largest tile, else the largest tile
  const int whole = sug_divup(E, REV_BLOCK) * REV_BLOCK;
  const int T = tile ? tile : (whole < SUG_REV_TILED_MAX_TILE ? whole : SUG_REV_TILED_MAX_TILE);
  hipStream_t st = (hipStream_t)stream;
  if (T <= 8 * REV_BLOCK) return reverse_lists_tiled_launch<8>(idx, B, E, N, RS, T, rev_off, rev_ent, st);
  return reverse_lists_tiled_launch<20>(idx, B, E, N, RS, T, rev_off, rev_ent, st);
}
