// Point Feature Histograms and the histogram cloud distance of the reference's utils/pfh.py (PFH.calc_normals,
// PFH.calcHistArray, pfh_hist_distance), M clouds or B (source, target) pairs per launch, one workgroup per cloud / pair.
// Semantics: include/sug_amd.h.
//
// sug_pfh_descriptors: the cloud sits in LDS as fp64 SoA and is swept with broadcast reads; every lane OWNS the points
// t, t + 256, ... through three phases separated by two barriers: (1) its neighbour list, by k + 1 sweeps that each take the
// least (distance, index) above the previous one -- nothing to sort, nothing indexed at run time in registers -- and from
// the list the PCA normal (cyclic Jacobi on the 3x3 covariance); (2) the Darboux features of the pairs of [i] + neighbours,
// binned into byte counters in LDS, one column per lane; (3) the row = counts / comb(k + 1, 2).
// sug_pfh_hist_distance: every lane owns source rows, sweeps the target rows (the same address in every lane), leaves its
// minima in LDS; the median is the element(s) of rank (n - 1) / 2 and n / 2, ranks by counting.
// No atomics, no fma (the Makefile compiles with -ffp-contract=off), every sum in one fixed order.
#include "common.h"

namespace {

constexpr int PFH_THREADS = 256;
constexpr int PFH_WAVES = PFH_THREADS / WAVE;
constexpr int PFH_MAX_POINTS = SUG_PFH_MAX_POINTS;
constexpr int PFH_MAX_K = SUG_PFH_MAX_NEIGHBORS;
constexpr int PFH_MAX_DIV = 5;
constexpr int PFH_JACOBI_SWEEPS = 12;                           // hard cap; a symmetric 3x3 converges in 4-6 sweeps
static_assert(PFH_MAX_POINTS <= 65535, "neighbour indices are kept as 16-bit values in LDS");
static_assert((PFH_MAX_K + 1) * PFH_MAX_K / 2 <= 255, "the bin counters are bytes");

struct PfhArgs {
  const float* pts;
  int N, k, div;
  double rad, npairs;
  double thr[3][PFH_MAX_DIV - 1];                               // thresholds of alpha, phi, theta (calc_thresholds)
  double* hist;
  double* normals;
  int32_t* nbr_idx;
  int32_t* nbr_cnt;
  int32_t* used_cnt;
};

__device__ __forceinline__ double dot3d(double ax, double ay, double az, double bx, double by, double bz) {
  return (ax * bx + ay * by) + az * bz;
}

// One rotation of the cyclic Jacobi iteration on the symmetric matrix A (all nine entries kept) with the eigenvector
// accumulation V <- V G: zeroes A[P][Q].  P, Q compile-time, so everything stays in registers.  Returns whether it rotated.
template <int P, int Q>
__device__ __forceinline__ bool jacobi_sym(double (&A)[3][3], double (&V)[3][3]) {
  constexpr int R = 3 - P - Q;
  const double apq = A[P][Q], app = A[P][P], aqq = A[Q][Q];
  // already diagonal to rounding (also: an exact zero)
  if (!(apq * apq > 1e-34 * fabs(app * aqq)) || apq == 0.0) return false;
  const double theta = (aqq - app) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(1.0 + theta * theta));
  const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
  A[P][P] = app - t * apq;
  A[Q][Q] = aqq + t * apq;
  A[P][Q] = 0.0; A[Q][P] = 0.0;
  const double arp = A[R][P], arq = A[R][Q];
  A[R][P] = c * arp - s * arq; A[P][R] = A[R][P];
  A[R][Q] = s * arp + c * arq; A[Q][R] = A[R][Q];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double u = V[r][P], v = V[r][Q];
    V[r][P] = c * u - s * v;
    V[r][Q] = s * u + c * v;
  }
  return true;
}

// step() of utils/pfh.py:441-479: the number of thresholds at or below f; a NaN lands in the last bin
__device__ __forceinline__ int pfh_step(const double (&thr)[PFH_MAX_DIV - 1], int div, double f) {
  if (f != f) return div - 1;
  int s = 0;
#pragma unroll
  for (int i = 0; i < PFH_MAX_DIV - 1; ++i) s += (i < div - 1 && f >= thr[i]) ? 1 : 0;
  return s;
}

__global__ __launch_bounds__(PFH_THREADS) void pfh_descriptors_kernel(const PfhArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  __shared__ int s_used[PFH_WAVES];
  const int m = blockIdx.x, t = threadIdx.x;
  const int N = a.N, k = a.k, div = a.div, D = div * div * div;
  double* px = reinterpret_cast<double*>(s_raw);
  double* py = px + N;
  double* pz = py + N;
  double* nx = pz + N;
  double* ny = nx + N;
  double* nz = ny + N;
  unsigned short* nbr = reinterpret_cast<unsigned short*>(nz + N);          // [N][k]
  unsigned char* cnt = reinterpret_cast<unsigned char*>(nbr + (size_t)N * k);   // [N]
  unsigned char* bins = cnt + ((N + 15) & ~15);                             // [D][PFH_THREADS]

  const float* pb = a.pts + (int64_t)m * N * 3;
  for (int j = t; j < N; j += PFH_THREADS) {
    px[j] = (double)pb[3 * j + 0]; py[j] = (double)pb[3 * j + 1]; pz[j] = (double)pb[3 * j + 2];
  }
  __syncthreads();

  // ---- phase 1: neighbours and normal of every owned point
  int used = 0;
  for (int i = t; i < N; i += PFH_THREADS) {
    const double x = px[i], y = py[i], z = pz[i];
    double pd = -1.0;                                             // the previous pick: every candidate lies above it
    int pj = -1, found = 0;
    int32_t* gi = a.nbr_idx + ((int64_t)m * N + i) * k;
    for (int r = 0; r <= k; ++r) {
      double bd = INFINITY;
      int bj = -1;
      for (int j = 0; j < N; ++j) {                               // the same address in every lane: LDS broadcast
        const double dx = x - px[j], dy = y - py[j], dz = z - pz[j];
        const double d = sqrt((dx * dx + dy * dy) + dz * dz);
        // within the radius (a NaN never is), after the previous pick in (distance, index), and before the best so far:
        // strict, so the lowest index keeps a tie
        if (d <= a.rad && (d > pd || (d == pd && j > pj)) && d < bd) { bd = d; bj = j; }
      }
      if (bj < 0) break;
      pd = bd; pj = bj;
      if (r > 0) {                                                // the first of the order is dropped (normally i itself)
        nbr[(size_t)i * k + found] = (unsigned short)bj;
        gi[found] = bj;
        ++found;
      }
    }
    for (int r = found; r < k; ++r) gi[r] = -1;
    cnt[i] = (unsigned char)found;
    a.nbr_cnt[(int64_t)m * N + i] = found;
    double nrm[3] = {0.0, 0.0, 0.0};
    if (found > 0) {
      ++used;
      double sx = 0.0, sy = 0.0, sz = 0.0;
      for (int r = 0; r < found; ++r) {
        const int j = nbr[(size_t)i * k + r];
        sx += px[j]; sy += py[j]; sz += pz[j];
      }
      const double n = (double)found;
      const double mx = sx / n, my = sy / n, mz = sz / n;
      double cxx = 0.0, cxy = 0.0, cxz = 0.0, cyy = 0.0, cyz = 0.0, czz = 0.0;
      for (int r = 0; r < found; ++r) {
        const int j = nbr[(size_t)i * k + r];
        const double ex = px[j] - mx, ey = py[j] - my, ez = pz[j] - mz;
        cxx += ex * ex; cxy += ex * ey; cxz += ex * ez; cyy += ey * ey; cyz += ey * ez; czz += ez * ez;
      }
      double A[3][3] = {{cxx / n, cxy / n, cxz / n}, {cxy / n, cyy / n, cyz / n}, {cxz / n, cyz / n, czz / n}};
      double V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
      for (int sweep = 0; sweep < PFH_JACOBI_SWEEPS; ++sweep) {
        bool any = jacobi_sym<0, 1>(A, V);
        any |= jacobi_sym<0, 2>(A, V);
        any |= jacobi_sym<1, 2>(A, V);
        if (!any) break;
      }
      // the column of the smallest eigenvalue, ties -> lowest index (by selects: no run-time subscript)
      const double l0 = A[0][0], l1 = A[1][1], l2 = A[2][2];
      const int c = (l0 <= l1 && l0 <= l2) ? 0 : (l1 <= l2 ? 1 : 2);
#pragma unroll
      for (int r = 0; r < 3; ++r) nrm[r] = c == 0 ? V[r][0] : (c == 1 ? V[r][1] : V[r][2]);
      // re-orient (utils/pfh.py:297): negate when normal . (-p) < 0
      if (dot3d(nrm[0], nrm[1], nrm[2], -x, -y, -z) < 0.0) { nrm[0] = -nrm[0]; nrm[1] = -nrm[1]; nrm[2] = -nrm[2]; }
    }
    nx[i] = nrm[0]; ny[i] = nrm[1]; nz[i] = nrm[2];
    double* gn = a.normals + ((int64_t)m * N + i) * 3;
    gn[0] = nrm[0]; gn[1] = nrm[1]; gn[2] = nrm[2];
  }
  // used points of the cloud: lanes, then waves, in a fixed order (integers: any order gives the same sum)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) used += __shfl_xor(used, o);
  if ((t & (WAVE - 1)) == 0) s_used[t / WAVE] = used;
  __syncthreads();                                                // normals, lists and s_used are complete
  if (t == 0) {
    int u = 0;
#pragma unroll
    for (int w = 0; w < PFH_WAVES; ++w) u += s_used[w];
    a.used_cnt[m] = u;
  }

  // ---- phase 2 and 3: pair features into this lane's column of byte counters, then the row
  for (int i = t; i < N; i += PFH_THREADS) {
    for (int b = 0; b < D; ++b) bins[b * PFH_THREADS + t] = 0;
    const int len = (int)cnt[i] + 1;                              // p_list = [i] + neighbours
    for (int zi = 0; zi + 1 < len; ++zi) {
      const int z = zi == 0 ? i : (int)nbr[(size_t)i * k + zi - 1];
      const double zx = px[z], zy = py[z], zz = pz[z], znx = nx[z], zny = ny[z], znz = nz[z];
      for (int pi = zi + 1; pi < len; ++pi) {
        const int p = nbr[(size_t)i * k + pi - 1];
        const double qx = px[p], qy = py[p], qz = pz[p], qnx = nx[p], qny = ny[p], qnz = nz[p];
        // arccos(n_p . (p_z - p_p)) <= arccos(n_z . (p_p - p_z)): both arguments in [-1, 1] (else a NaN: false) and a >= b
        const double ca = dot3d(qnx, qny, qnz, zx - qx, zy - qy, zz - qz);
        const double cb = dot3d(znx, zny, znz, qx - zx, qy - zy, qz - zz);
        const bool p_src = fabs(ca) <= 1.0 && fabs(cb) <= 1.0 && ca >= cb;
        const double sx = p_src ? qx : zx, sy = p_src ? qy : zy, sz = p_src ? qz : zz;
        const double tx = p_src ? zx : qx, ty = p_src ? zy : qy, tz = p_src ? zz : qz;
        const double ux = p_src ? qnx : znx, uy = p_src ? qny : zny, uz = p_src ? qnz : znz;
        const double wx = p_src ? znx : qnx, wy = p_src ? zny : qny, wz = p_src ? znz : qnz;      // n_t
        double dx = tx - sx, dy = ty - sy, dz = tz - sz;
        const double dist = sqrt(dot3d(dx, dy, dz, dx, dy, dz));
        dx = dx / dist; dy = dy / dist; dz = dz / dist;           // a zero distance: NaN features, the last bin
        const double vx = dy * uz - dz * uy, vy = dz * ux - dx * uz, vz = dx * uy - dy * ux;       // v = d x u
        const double hx = uy * vz - uz * vy, hy = uz * vx - ux * vz, hz = ux * vy - uy * vx;       // w = u x v
        const double alpha = dot3d(vx, vy, vz, wx, wy, wz);
        const double phi = dot3d(ux, uy, uz, dx, dy, dz);
        const double theta = atan(dot3d(hx, hy, hz, wx, wy, wz) / dot3d(ux, uy, uz, wx, wy, wz));
        const int bin = pfh_step(a.thr[0], div, alpha) + div * pfh_step(a.thr[1], div, phi) +
                        div * div * pfh_step(a.thr[2], div, theta);
        bins[bin * PFH_THREADS + t] += 1;
      }
    }
    double* gh = a.hist + ((int64_t)m * N + i) * D;
    for (int b = 0; b < D; ++b) gh[b] = (double)bins[b * PFH_THREADS + t] / a.npairs;
  }
}

struct PfhDistArgs {
  const double* hs;
  const int32_t* cs;
  int64_t hs_stride, cs_stride;
  const double* ht;
  const int32_t* ct;
  int Ns, Nt, D;
  double* out;
};

// DR > 0: D == DR, the owned source row is held in registers; DR == 0: any D, the row is re-read (it stays in L1)
template <int DR>
__global__ __launch_bounds__(PFH_THREADS) void pfh_hist_distance_kernel(const PfhDistArgs a) {
  __shared__ double s_min[PFH_MAX_POINTS];
  __shared__ unsigned char s_use[PFH_MAX_POINTS];
  __shared__ double s_mid[2];
  const int b = blockIdx.x, t = threadIdx.x;
  const int Ns = a.Ns, Nt = a.Nt, D = DR > 0 ? DR : a.D;
  const double* hs = a.hs + (int64_t)b * a.hs_stride;
  const int32_t* cs = a.cs + (int64_t)b * a.cs_stride;
  const double* ht = a.ht + (int64_t)b * Nt * D;
  const int32_t* ct = a.ct + (int64_t)b * Nt;
  if (t < 2) s_mid[t] = NAN;
  for (int i = t; i < Ns; i += PFH_THREADS) {
    const bool use = cs[i] > 0;
    const double* row = hs + (int64_t)i * D;
    double reg[DR > 0 ? DR : 1];
    if (DR > 0) {
#pragma unroll
      for (int d = 0; d < DR; ++d) reg[d] = row[d];
    }
    double best = INFINITY;
    if (use) {
      for (int j = 0; j < Nt; ++j) {                              // wave-uniform: every lane reads the same target row
        if (ct[j] <= 0) continue;
        const double* tr = ht + (int64_t)j * D;
        double s = 0.0;
        if (DR > 0) {
#pragma unroll
          for (int d = 0; d < DR; ++d) { const double e = reg[d] - tr[d]; s += e * e; }
        } else {
          for (int d = 0; d < D; ++d) { const double e = row[d] - tr[d]; s += e * e; }
        }
        const double v = sqrt(s);
        if (v < best) best = v;
      }
    }
    s_min[i] = best;
    s_use[i] = use && best < INFINITY;                            // no used target row: no minimum
  }
  __syncthreads();
  // the median by ranks: rank of a used minimum = how many used minima come before it in (value, index)
  for (int i = t; i < Ns; i += PFH_THREADS) {
    if (!s_use[i]) continue;
    const double v = s_min[i];
    int rank = 0, n = 0;
    for (int j = 0; j < Ns; ++j) {
      if (!s_use[j]) continue;
      const double w = s_min[j];
      ++n;
      rank += (w < v || (w == v && j < i)) ? 1 : 0;
    }
    if (rank == (n - 1) / 2) s_mid[0] = v;                        // ranks are a permutation: one writer per slot
    if (rank == n / 2) s_mid[1] = v;
  }
  __syncthreads();
  if (t == 0) a.out[b] = (s_mid[0] + s_mid[1]) / 2.0;             // np.median: the mean of the two middle values; NaN if none
}

SugLdsOptIn g_pfh_lds;

}  // namespace

extern "C" int sug_pfh_descriptors(const float* pts, int M, int N, double rad, int nneighbors, int div, double* hist,
                                   double* normals, int32_t* nbr_idx, int32_t* nbr_cnt, int32_t* used_cnt, void* stream) {
  SUG_REQUIRE(pts && hist && normals && nbr_idx && nbr_cnt && used_cnt, "sug_pfh_descriptors: null pointer");
  SUG_REQUIRE(M > 0, "sug_pfh_descriptors: M=%d: an empty batch", M);
  SUG_REQUIRE(N >= 1 && N <= PFH_MAX_POINTS, "sug_pfh_descriptors: N=%d: 1 .. %d points per cloud", N, PFH_MAX_POINTS);
  SUG_REQUIRE(nneighbors >= 1 && nneighbors <= PFH_MAX_K, "sug_pfh_descriptors: nneighbors=%d outside 1 .. %d", nneighbors,
              PFH_MAX_K);
  SUG_REQUIRE(div >= 2 && div <= PFH_MAX_DIV, "sug_pfh_descriptors: div=%d outside 2 .. %d", div, PFH_MAX_DIV);
  SUG_REQUIRE(rad > 0.0 && rad < INFINITY, "sug_pfh_descriptors: rad=%g must be positive and finite", rad);
  PfhArgs a;
  a.pts = pts; a.N = N; a.k = nneighbors; a.div = div; a.rad = rad;
  a.npairs = (double)((nneighbors + 1) * nneighbors / 2);         // comb(k + 1, 2), the configured k (utils/pfh.py:311)
  // calc_thresholds (utils/pfh.py:481-495), the same operations in the same order
  const double delta = 2.0 / div, delta_t = M_PI / div;
  for (int i = 0; i < PFH_MAX_DIV - 1; ++i) {
    a.thr[0][i] = a.thr[1][i] = i < div - 1 ? -1.0 + (i + 1) * delta : INFINITY;
    a.thr[2][i] = i < div - 1 ? -M_PI / 2.0 + (i + 1) * delta_t : INFINITY;
  }
  a.hist = hist; a.normals = normals; a.nbr_idx = nbr_idx; a.nbr_cnt = nbr_cnt; a.used_cnt = used_cnt;
  // points and normals as fp64 SoA, the lists, the counts, the byte counters: <= 112 KB of the CU's 160
  const size_t sh = (size_t)N * 6 * sizeof(double) + (size_t)N * nneighbors * sizeof(unsigned short) + (size_t)((N + 15) & ~15) +
                    (size_t)div * div * div * PFH_THREADS;
  if (sh > 48 * 1024) {
    const int rc = sug_allow_dynamic_lds(g_pfh_lds, pfh_descriptors_kernel, (int)sh, "sug_pfh_descriptors");
    if (rc != SUG_OK) return rc;
  }
  hipLaunchKernelGGL(pfh_descriptors_kernel, dim3(M), dim3(PFH_THREADS), sh, (hipStream_t)stream, a);
  SUG_LAUNCH_CHECK("sug_pfh_descriptors");
  return SUG_OK;
}

extern "C" int sug_pfh_hist_distance(const double* histS, const int32_t* cntS, int64_t src_batch_stride, const double* histT,
                                     const int32_t* cntT, int B, int Ns, int Nt, int D, double* out, void* stream) {
  SUG_REQUIRE(histS && cntS && histT && cntT && out, "sug_pfh_hist_distance: null pointer");
  SUG_REQUIRE(B > 0, "sug_pfh_hist_distance: B=%d: an empty batch", B);
  SUG_REQUIRE(Ns >= 1 && Ns <= PFH_MAX_POINTS && Nt >= 1 && Nt <= PFH_MAX_POINTS,
              "sug_pfh_hist_distance: Ns=%d, Nt=%d: 1 .. %d rows per cloud", Ns, Nt, PFH_MAX_POINTS);
  SUG_REQUIRE(D == 8 || D == 27 || D == 64 || D == 125, "sug_pfh_hist_distance: D=%d is not div^3 of a div in 2 .. %d", D,
              PFH_MAX_DIV);
  SUG_REQUIRE(src_batch_stride == 0 || src_batch_stride == (int64_t)Ns * D,
              "sug_pfh_hist_distance: src_batch_stride=%lld: 0 (one source for all pairs) or Ns*D=%lld",
              (long long)src_batch_stride, (long long)Ns * D);
  PfhDistArgs a;
  a.hs = histS; a.cs = cntS; a.hs_stride = src_batch_stride; a.cs_stride = src_batch_stride == 0 ? 0 : Ns;
  a.ht = histT; a.ct = cntT; a.Ns = Ns; a.Nt = Nt; a.D = D; a.out = out;
  hipStream_t st = (hipStream_t)stream;
  switch (D) {
    case 8: hipLaunchKernelGGL(pfh_hist_distance_kernel<8>, dim3(B), dim3(PFH_THREADS), 0, st, a); break;
    case 27: hipLaunchKernelGGL(pfh_hist_distance_kernel<27>, dim3(B), dim3(PFH_THREADS), 0, st, a); break;
    case 64: hipLaunchKernelGGL(pfh_hist_distance_kernel<64>, dim3(B), dim3(PFH_THREADS), 0, st, a); break;
    default: hipLaunchKernelGGL(pfh_hist_distance_kernel<0>, dim3(B), dim3(PFH_THREADS), 0, st, a); break;
  }
  SUG_LAUNCH_CHECK("sug_pfh_hist_distance");
  return SUG_OK;
}
