// Batched point-to-point ICP fitness: the registration loop behind icp_distance() of the sub-domain splitter
// (dataset_splitter.py:217-231, open3d's registration_icp with its defaults), B independent (source, target) pairs in
// one launch, one workgroup per pair.  Semantics and assumptions: include/sug_amd.h.
//
// The target sits in LDS as fp64 SoA and is swept with broadcast reads; every lane OWNS up to 4 source points (PPL)
// and keeps them, cumulatively transformed, in registers (nobody else reads them).  Per evaluation one block reduction
// in a fixed order (xor butterflies inside a wave, then the waves in index order from LDS) yields the 17 sums
// count, sum d2, sum p, sum q, sum p q^T; every lane folds the same LDS values in the same order, so the update, the
// stopping test and the loop exit are workgroup-uniform by construction.  No atomics, no fma (the Makefile compiles with
// -ffp-contract=off): products and sums round one by one.
#include "common.h"

namespace {

constexpr int ICP_THREADS = 256;
constexpr int ICP_WAVES = ICP_THREADS / WAVE;
constexpr int ICP_MAX_POINTS = SUG_ICP_MAX_POINTS;
static_assert(ICP_MAX_POINTS <= 4 * ICP_THREADS, "the launcher instantiates 1 .. 4 source points per lane");
constexpr int ICP_MAX_ITER = 64;
constexpr int ICP_SUMS = 17;
constexpr int ICP_JACOBI_SWEEPS = 12;                           // hard cap; a 3x3 converges in 4-6 sweeps

struct IcpSums {
  double cnt, sd2, p[3], q[3], pq[3][3];                        // pq[r][c] = sum q_r p_c
};

// One Jacobi rotation of the columns (a, b) of the 3x3 pair (A, V): makes the columns of A orthogonal.  Returns whether it
// rotated.  One-sided (Hestenes) Jacobi: A V' = U S with A the input, V' the accumulated rotations.
__device__ __forceinline__ bool jacobi_pair(double A[3][3], double V[3][3], int a, int b) {
  const double alpha = (A[0][a] * A[0][a] + A[1][a] * A[1][a]) + A[2][a] * A[2][a];
  const double beta = (A[0][b] * A[0][b] + A[1][b] * A[1][b]) + A[2][b] * A[2][b];
  const double gamma = (A[0][a] * A[0][b] + A[1][a] * A[1][b]) + A[2][a] * A[2][b];
  // already orthogonal to rounding (also: a zero column, or products that underflowed)
  if (!(gamma * gamma > 1e-30 * (alpha * beta))) return false;
  const double zeta = (beta - alpha) / (2.0 * gamma);
  const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
  const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double x = A[r][a], y = A[r][b];
    A[r][a] = c * x - s * y;
    A[r][b] = s * x + c * y;
    const double u = V[r][a], v = V[r][b];
    V[r][a] = c * u - s * v;
    V[r][b] = s * u + c * v;
  }
  return true;
}

// column i of a 3x3 held in registers, by selects (a run-time subscript would put the matrix into scratch)
__device__ __forceinline__ double pick3(double x0, double x1, double x2, int i) { return i == 0 ? x0 : (i == 1 ? x1 : x2); }

__device__ __forceinline__ void cross3(const double a[3], const double b[3], double o[3]) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

// a unit vector orthogonal to the unit vector u: the coordinate axis least aligned with u, made orthogonal to it
__device__ __forceinline__ void any_orthogonal(const double u[3], double o[3]) {
  const double ax = fabs(u[0]), ay = fabs(u[1]), az = fabs(u[2]);
  const int ax0 = (ax <= ay && ax <= az) ? 0 : (ay <= az ? 1 : 2);
  const double e[3] = {ax0 == 0 ? 1.0 : 0.0, ax0 == 1 ? 1.0 : 0.0, ax0 == 2 ? 1.0 : 0.0};
  const double d = (e[0] * u[0] + e[1] * u[1]) + e[2] * u[2];
  double n2 = 0.0;
#pragma unroll
  for (int r = 0; r < 3; ++r) { o[r] = e[r] - d * u[r]; n2 += o[r] * o[r]; }
  const double inv = 1.0 / sqrt(n2);              // n2 >= 2/3
#pragma unroll
  for (int r = 0; r < 3; ++r) o[r] *= inv;
}

// The update of TransformationEstimationPointToPoint (Umeyama without scaling) from the 17 sums:
// R = U diag(1, 1, sign(det U det V)) V^T of Sigma = U S V^T, t = qbar - R pbar.
// With (u1, v1), (u2, v2) the singular pairs of the two largest singular values, det(U) u3 = u1 x u2 and
// det(V) v3 = v1 x v2 whatever the sign the decomposition gave u3 and v3, so
//     R = u1 v1^T + u2 v2^T + (u1 x u2)(v1 x v2)^T
// is that formula without its third singular vector, which is the ill-determined one when Sigma loses rank: R is a
// proper rotation (orthonormal pairs in, det +1 out) for every Sigma.  Rank 2 gives what Umeyama prescribes there.
// Rank 1: the rotation about the one determined axis is arbitrary; (u2, v2) is an orthogonal completion -- the one
// any_orthogonal() picks when the second column vanishes, else the direction rounding left in it.  Rank 0 (all
// correspondences on one point, Sigma exactly 0): R = I, a pure translation.
__device__ void icp_update(const IcpSums& s, double R[3][3], double t[3]) {
  const double n = s.cnt, inv_n = 1.0 / n;
  double pm[3], qm[3], A[3][3], V[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r) { pm[r] = s.p[r] * inv_n; qm[r] = s.q[r] * inv_n; }
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      A[r][c] = s.pq[r][c] * inv_n - qm[r] * pm[c];
      V[r][c] = r == c ? 1.0 : 0.0;
    }
  for (int sweep = 0; sweep < ICP_JACOBI_SWEEPS; ++sweep) {
    bool any = jacobi_pair(A, V, 0, 1);
    any |= jacobi_pair(A, V, 0, 2);
    any |= jacobi_pair(A, V, 1, 2);
    if (!any) break;
  }
  double sg[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) sg[c] = (A[0][c] * A[0][c] + A[1][c] * A[1][c]) + A[2][c] * A[2][c];   // sigma^2
  // columns of the largest (i1) and second largest (i2) singular value, ties -> lowest index
  const int i1 = (sg[0] >= sg[1] && sg[0] >= sg[2]) ? 0 : (sg[1] >= sg[2] ? 1 : 2);
  const int ja = i1 == 0 ? 1 : 0, jb = i1 == 2 ? 1 : 2;
  const double sga = pick3(sg[0], sg[1], sg[2], ja), sgb = pick3(sg[0], sg[1], sg[2], jb);
  const int i2 = sga >= sgb ? ja : jb;
  double u1[3], u2[3], v1[3], v2[3], u3[3], v3[3];
  const double s1 = pick3(sg[0], sg[1], sg[2], i1), s2 = sga >= sgb ? sga : sgb;
  // a column counts as zero below 1e-14 of the largest singular value (sigma^2 below 1e-28 of the largest).  That catches
  // an exactly vanishing column only: Sigma comes from raw sums, whose cancellation leaves about 1e-16 ABSOLUTE, so for
  // close correspondences (sigma_1 small) the residue of a rank-1 Sigma can lie above the threshold and is then used as
  // the second direction.  Harmless: the Jacobi columns are orthogonal, so (u2, v2) is a valid completion either way;
  // which one it is, is then set by rounding (deterministically), not by any_orthogonal()
  const bool has1 = s1 > 1e-300, has2 = has1 && s2 > 1e-28 * s1;
  if (has1) {
    const double inv = 1.0 / sqrt(s1);
#pragma unroll
    for (int r = 0; r < 3; ++r) { u1[r] = pick3(A[r][0], A[r][1], A[r][2], i1) * inv; v1[r] = pick3(V[r][0], V[r][1], V[r][2], i1); }
  } else {
    u1[0] = v1[0] = 1.0; u1[1] = v1[1] = 0.0; u1[2] = v1[2] = 0.0;
  }
  if (has2) {
    const double inv = 1.0 / sqrt(s2);
#pragma unroll
    for (int r = 0; r < 3; ++r) { u2[r] = pick3(A[r][0], A[r][1], A[r][2], i2) * inv; v2[r] = pick3(V[r][0], V[r][1], V[r][2], i2); }
  } else {
    any_orthogonal(u1, u2);
    any_orthogonal(v1, v2);
  }
  cross3(u1, u2, u3);
  cross3(v1, v2, v3);
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) R[r][c] = (u1[r] * v1[c] + u2[r] * v2[c]) + u3[r] * v3[c];
#pragma unroll
  for (int r = 0; r < 3; ++r) t[r] = qm[r] - ((R[r][0] * pm[0] + R[r][1] * pm[1]) + R[r][2] * pm[2]);
}

struct IcpArgs {
  const float* src;
  const float* tgt;
  int64_t src_batch_stride;
  int Ns, Nt, max_iteration;
  double r2, rel_fitness, rel_rmse;
  int32_t* count;
  double* rmse;
  int32_t* iters;
  double* transform;
};

// evaluate(): nearest target of every owned point, then the block reduction of the 17 sums into `out` (identical in all
// lanes).  `buf` alternates between calls: a wave that writes s_part[buf] again has passed the barrier of the call in
// between, which every wave reaches only after it has read s_part[buf].  Contains one __syncthreads().
template <int PPL>
__device__ __forceinline__ void icp_evaluate(const double (&px)[PPL], const double (&py)[PPL], const double (&pz)[PPL],
                                             const bool (&own)[PPL], const double* tx, const double* ty,
                                             const double* tz, int Nt, double r2,
                                             double (*s_part)[ICP_WAVES][ICP_SUMS], int buf, IcpSums& out) {
  double best[PPL];
  int arg[PPL];
#pragma unroll
  for (int k = 0; k < PPL; ++k) { best[k] = INFINITY; arg[k] = 0; }
  for (int j = 0; j < Nt; ++j) {
    const double qx = tx[j], qy = ty[j], qz = tz[j];                 // the same address in every lane: LDS broadcast
#pragma unroll
    for (int k = 0; k < PPL; ++k) {
      const double dx = px[k] - qx, dy = py[k] - qy, dz = pz[k] - qz;
      const double d = (dx * dx + dy * dy) + dz * dz;
      if (d < best[k]) { best[k] = d; arg[k] = j; }                  // strict: the lowest index keeps a tie
    }
  }
  double v[ICP_SUMS];
#pragma unroll
  for (int i = 0; i < ICP_SUMS; ++i) v[i] = 0.0;
#pragma unroll
  for (int k = 0; k < PPL; ++k) {
    if (own[k] && best[k] < r2) {                                    // NaN coordinates never correspond
      const double qx = tx[arg[k]], qy = ty[arg[k]], qz = tz[arg[k]];
      v[0] += 1.0; v[1] += best[k];
      v[2] += px[k]; v[3] += py[k]; v[4] += pz[k];
      v[5] += qx; v[6] += qy; v[7] += qz;
      v[8] += qx * px[k]; v[9] += qx * py[k]; v[10] += qx * pz[k];
      v[11] += qy * px[k]; v[12] += qy * py[k]; v[13] += qy * pz[k];
      v[14] += qz * px[k]; v[15] += qz * py[k]; v[16] += qz * pz[k];
    }
  }
  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
#pragma unroll
  for (int i = 0; i < ICP_SUMS; ++i) {
    v[i] = wave_sum_d(v[i]);
    if (lane == 0) s_part[buf][wv][i] = v[i];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < ICP_SUMS; ++i) {
    double a = s_part[buf][0][i];
#pragma unroll
    for (int w = 1; w < ICP_WAVES; ++w) a += s_part[buf][w][i];
    v[i] = a;
  }
  out.cnt = v[0]; out.sd2 = v[1];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    out.p[r] = v[2 + r]; out.q[r] = v[5 + r];
#pragma unroll
    for (int c = 0; c < 3; ++c) out.pq[r][c] = v[8 + 3 * r + c];
  }
}

template <int PPL>
__global__ __launch_bounds__(ICP_THREADS) void icp_fitness_kernel(const IcpArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  __shared__ double s_part[2][ICP_WAVES][ICP_SUMS];
  const int b = blockIdx.x, t = threadIdx.x;
  const int Ns = a.Ns, Nt = a.Nt;
  double* tx = reinterpret_cast<double*>(s_raw);
  double* ty = tx + Nt;
  double* tz = ty + Nt;
  const float* tb = a.tgt + (int64_t)b * Nt * 3;
  for (int j = t; j < Nt; j += ICP_THREADS) {
    tx[j] = (double)tb[3 * j + 0]; ty[j] = (double)tb[3 * j + 1]; tz[j] = (double)tb[3 * j + 2];
  }
  const float* sb = a.src + (int64_t)b * a.src_batch_stride;
  double px[PPL], py[PPL], pz[PPL];
  bool own[PPL];
#pragma unroll
  for (int k = 0; k < PPL; ++k) {
    const int i = t + k * ICP_THREADS;
    own[k] = i < Ns;
    px[k] = own[k] ? (double)sb[3 * i + 0] : 0.0;
    py[k] = own[k] ? (double)sb[3 * i + 1] : 0.0;
    pz[k] = own[k] ? (double)sb[3 * i + 2] : 0.0;
  }
  __syncthreads();

  double T[3][4] = {{1.0, 0.0, 0.0, 0.0}, {0.0, 1.0, 0.0, 0.0}, {0.0, 0.0, 1.0, 0.0}};     // rows 0..2 of the 4x4
  IcpSums s;
  int buf = 0;
  icp_evaluate<PPL>(px, py, pz, own, tx, ty, tz, Nt, a.r2, s_part, buf, s);
  buf ^= 1;
  double fitness = s.cnt / (double)Ns;
  double rmse = s.cnt > 0.0 ? sqrt(s.sd2 / s.cnt) : 0.0;
  int iters = 0;
  // every quantity the two exits below test was folded from the same LDS values in the same order by every lane, so the
  // whole workgroup leaves the loop (and skips the barrier inside icp_evaluate) together
  for (int it = 0; it < a.max_iteration; ++it) {
    if (s.cnt == 0.0) break;
    double R[3][3], tr[3];
    icp_update(s, R, tr);
#pragma unroll
    for (int k = 0; k < PPL; ++k) {
      const double x = px[k], y = py[k], z = pz[k];
      px[k] = ((R[0][0] * x + R[0][1] * y) + R[0][2] * z) + tr[0];
      py[k] = ((R[1][0] * x + R[1][1] * y) + R[1][2] * z) + tr[1];
      pz[k] = ((R[2][0] * x + R[2][1] * y) + R[2][2] * z) + tr[2];
    }
    double Tn[3][4];                                                 // transform = update . transform
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c)
        Tn[r][c] = ((R[r][0] * T[0][c] + R[r][1] * T[1][c]) + R[r][2] * T[2][c]) + (c == 3 ? tr[r] : 0.0);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) T[r][c] = Tn[r][c];
    ++iters;
    const double prev_fitness = fitness, prev_rmse = rmse;
    icp_evaluate<PPL>(px, py, pz, own, tx, ty, tz, Nt, a.r2, s_part, buf, s);
    buf ^= 1;
    fitness = s.cnt / (double)Ns;
    rmse = s.cnt > 0.0 ? sqrt(s.sd2 / s.cnt) : 0.0;
    if (fabs(prev_fitness - fitness) < a.rel_fitness && fabs(prev_rmse - rmse) < a.rel_rmse) break;
  }
  if (t == 0) {
    a.count[b] = (int32_t)s.cnt;
    a.rmse[b] = rmse;
    a.iters[b] = iters;
    double* o = a.transform + (int64_t)b * 16;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) o[4 * r + c] = T[r][c];
    o[12] = 0.0; o[13] = 0.0; o[14] = 0.0; o[15] = 1.0;
  }
}

}  // namespace

extern "C" int sug_icp_fitness(const float* src, int64_t src_batch_stride, const float* tgt, int B, int Ns, int Nt,
                               double max_corr_dist, int max_iteration, double rel_fitness, double rel_rmse,
                               int32_t* count, double* rmse, int32_t* iters, double* transform, void* stream) {
  SUG_REQUIRE(src && tgt && count && rmse && iters && transform, "sug_icp_fitness: null pointer");
  SUG_REQUIRE(B > 0, "sug_icp_fitness: B=%d: an empty batch", B);
  SUG_REQUIRE(Ns >= 1 && Ns <= ICP_MAX_POINTS && Nt >= 1 && Nt <= ICP_MAX_POINTS,
              "sug_icp_fitness: Ns=%d, Nt=%d: 1 .. %d points per cloud", Ns, Nt, ICP_MAX_POINTS);
  SUG_REQUIRE(max_iteration >= 0 && max_iteration <= ICP_MAX_ITER, "sug_icp_fitness: max_iteration=%d outside 0 .. %d",
              max_iteration, ICP_MAX_ITER);
  SUG_REQUIRE(max_corr_dist > 0.0 && max_corr_dist < INFINITY, "sug_icp_fitness: max_corr_dist=%g must be positive and finite",
              max_corr_dist);
  SUG_REQUIRE(src_batch_stride == 0 || src_batch_stride == 3 * (int64_t)Ns,
              "sug_icp_fitness: src_batch_stride=%lld: 0 (one source for all pairs) or 3*Ns=%d", (long long)src_batch_stride,
              3 * Ns);
  SUG_REQUIRE(rel_fitness == rel_fitness && rel_rmse == rel_rmse, "sug_icp_fitness: rel_fitness / rel_rmse is NaN");
  IcpArgs a;
  a.src = src; a.tgt = tgt; a.src_batch_stride = src_batch_stride;
  a.Ns = Ns; a.Nt = Nt; a.max_iteration = max_iteration;
  a.r2 = max_corr_dist * max_corr_dist; a.rel_fitness = rel_fitness; a.rel_rmse = rel_rmse;
  a.count = count; a.rmse = rmse; a.iters = iters; a.transform = transform;
  const size_t sh = (size_t)Nt * 3 * sizeof(double);                 // <= 24 KB
  const int ppl = sug_divup(Ns, ICP_THREADS);
  hipStream_t st = (hipStream_t)stream;
  switch (ppl) {
    case 1: hipLaunchKernelGGL(icp_fitness_kernel<1>, dim3(B), dim3(ICP_THREADS), sh, st, a); break;
    case 2: hipLaunchKernelGGL(icp_fitness_kernel<2>, dim3(B), dim3(ICP_THREADS), sh, st, a); break;
    case 3: hipLaunchKernelGGL(icp_fitness_kernel<3>, dim3(B), dim3(ICP_THREADS), sh, st, a); break;
    default: hipLaunchKernelGGL(icp_fitness_kernel<4>, dim3(B), dim3(ICP_THREADS), sh, st, a); break;
  }
  SUG_LAUNCH_CHECK("sug_icp_fitness");
  return SUG_OK;
}
