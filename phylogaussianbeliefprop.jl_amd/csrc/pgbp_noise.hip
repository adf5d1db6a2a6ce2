// Measurement error at the tips in the factor fill (pgbp_lg_set_tip_noise of include/pgbp.h).
//
// A tip family f (child_pos < 0, a data row) with noise has the conditional variance V + E, E = scale_f Sigma_e + diag(se2_f):
// the tip's variable is the observation y = x + eps.  Means, qc, wc and the shifts do not change.  Notation of pgbp_lgfill.hip
// and pgbp_shift.hip: O = child_mask[f], c_0 = 1, c_k = -qc_k, z = w - sum over the fixed nodes of c_a y_a as the fill forms it,
// delta = d_O the displacement of the shifts, zt = z + delta; j = V_OO^-1, j' = (V_OO + E_OO)^-1 and
//     D = j' - j = -j E_OO j'          (formed as this product, never as a difference of two inverses).
// The family's factor changes by
//     Delta J_ab = c_a c_b D                       at the kept traits of the in-scope parents a, b,
//     Delta h_a  = c_a D zt,
//     Delta g    = -zt' D zt / 2 - (log det(V_OO + E_OO) - log det V_OO) / 2.
// The three fill kernels and the shift correction are left alone: these kernels run after them whenever noise is set.  One
// workgroup (one wavefront) per (cluster that holds a noisy tip family, site) walks the cluster's families in table order,
// eliminates [V_OO | E_OO | zt] and [V_OO + E_OO | I | zt] in LDS, accumulates the cluster's Delta J, Delta h, Delta g in LDS in
// family order and adds them to the record once: one writer per record, no atomics, every sum in a fixed order -- the same
// bytes on every call.  In the packed (BS16) layout both triangles of the diagonal 2 x 2 blocks are written; Delta J is exactly
// symmetric (the upper triangle of D mirrored), so they keep agreeing as far as the fill left them.  Nothing is launched when
// no noise is set.  A pivot of V_OO + E_OO (or of V_OO) that is not positive makes the record's g NaN.
//
// KNOWN LIMIT.  The fill writes j, the correction adds D ~ -j when |E| >> |V|: the sum j' carries an error of about
// eps (1 + |E| / |V|) relative to itself in the tip's contribution (eps = 2^-52).  At |E| / |V| = 1e7 about 1e-8 is left
// (tests/test_tip_noise_cpu.py prints the table; README).  Nothing is lost for |E| <= |V|.
#include <hip/hip_runtime.h>

#include "pgbp_bs16.hpp"
#include "pgbp_fam_dev.hpp"
#include "pgbp_kernels.hpp"
#include "pgbp_noise_dev.hpp"

namespace pgbp {

extern __shared__ double noise_lds[];

// Gauss-Jordan on the n x nc system [A | B] (row stride ld) in LDS by one wavefront: the right part becomes A^-1 B; logdet:
// log det A.  false when a pivot is not positive.  (lg_gauss_jordan of pgbp_lgfill.hip, for this file's systems.)
__device__ __forceinline__ bool noise_gauss_jordan(double* W, int n, int nc, int ld, int lane, double& logdet) {
  double mant = 1.0;
  int expo = 0;
  for (int k = 0; k < n; ++k) {
    const double d = W[k * ld + k];
    if (!(d > 0.0)) return false;
    int ex;
    mant *= frexp(d, &ex);
    expo += ex;
    const double rd = 1.0 / d;
    __syncthreads();
    for (int j = k + 1 + lane; j < nc; j += kWave) W[k * ld + j] *= rd;
    __syncthreads();
    const int ncol = nc - (k + 1);
    for (int idx = lane; idx < (n - 1) * ncol; idx += kWave) {
      int i = idx / ncol;
      const int j = k + 1 + (idx - i * ncol);
      if (i >= k) ++i;
      W[i * ld + j] -= W[i * ld + k] * W[k * ld + j];
    }
    __syncthreads();
  }
  logdet = log(mant) + (double)expo * 0.69314718055994530941723212145818;
  return true;
}

// LDS of noise_kernel in doubles: the accumulator [Delta J (m*m) | Delta h (m) | Delta g] of the largest noisy cluster, the two
// systems, c_a, then the ints (positions, kept traits)
__host__ __device__ inline int noise_ld(int p) { return (2 * p + 1) | 1; }
__host__ __device__ inline size_t noise_acc_cap(int m) { return ((size_t)m * m + m + 1 + 1) & ~(size_t)1; }
inline size_t noise_lds_doubles(int p, int K, int max_dim) {
  return noise_acc_cap(max_dim) + 2 * (size_t)p * noise_ld(p) + (size_t)(K + 1) + (size_t)(K + 2 + p) / 2 + 2;
}
size_t lg_noise_lds_bytes(int p, int K, int max_dim_ncl) { return sizeof(double) * noise_lds_doubles(p, K, max_dim_ncl); }

// plain and BS16 packed records.  ncl: the clusters that hold a noisy tip family; acc_cap: doubles kept for the accumulator
__global__ __launch_bounds__(64) void noise_kernel(LgStatic F, LgParams M, LgShifts S, LgOptima Op, LgNoise Nz,
                                                   const int32_t* __restrict__ ncl,
                                                   double* __restrict__ pool, int64_t pool_stride, double* __restrict__ fpool,
                                                   int64_t fpool_stride, const int64_t* __restrict__ boff,
                                                   const int32_t* __restrict__ dim, int bs, int fp, int acc_cap) {
  const int lane = threadIdx.x, c = ncl[blockIdx.x], site = blockIdx.y;
  const int p = F.p, K = F.K;
  const int m = dim[c];
  const int nrec = m * m + m + 1;
  double* __restrict__ out = pool + (int64_t)site * pool_stride + boff[c];
  double* __restrict__ fout = fpool ? fpool + (int64_t)site * fpool_stride + boff[c] : nullptr;
  double* acc = noise_lds;             // plain column-major [Delta J | Delta h | Delta g]
  const int ldmax = noise_ld(p);
  double* W1 = noise_lds + acc_cap;    // mo x ld: [V_OO | E_OO | zt]      -> [D (upper) | j E_OO | D zt]
  double* W2 = W1 + p * ldmax;         // mo x ld: [V_OO + E_OO | I | zt]  -> [. | j' | j' zt]
  double* cz = W2 + p * ldmax;         // c_a (K + 1)
  int* ipos = reinterpret_cast<int*>(cz + (K + 1));   // positions (K + 1), then the kept traits (p)
  int* oidx = ipos + (K + 1);
  for (int t = lane; t < nrec; t += kWave) acc[t] = 0.0;
  const int64_t ps = M.per_site ? site : 0;
  const double* __restrict__ R = M.R + ps * F.n_rates * p * p;
  const double* __restrict__ mu = M.mu + ps * p;
  const double* __restrict__ theta = M.theta ? M.theta + ps * p : nullptr;
  const double alpha = (M.model == PGBP_LG_OU) ? M.alpha[ps] : 0.0;
  const unsigned long long full = p >= 64 ? ~0ull : ((1ull << p) - 1ull);
  bool bad = false;
  for (int fi = F.cl_off[c]; fi < F.cl_off[c + 1]; ++fi) {
    const int f = F.cl_fam[fi];
    const int sn = Nz.slot[f];
    if (sn < 0) continue;             // (the same in every lane)
    const int np = F.n_parents[f];
    const unsigned long long O = F.child_mask ? (F.child_mask[f] & full) : full;
    const int mo = __popcll(O);
    if (mo == 0) continue;            // the factor is 1: nothing is observed
    const int nc = 2 * mo + 1, ld = nc | 1;
    __syncthreads();
    if (lane <= np) {
      if (lane == 0) {
        cz[0] = 1.0;
        ipos[0] = -1;                 // a tip: the child is data
      } else {
        double qc, vc, wc;
        lg_coefs<true>(M.model, alpha, F.length[(int64_t)f * K + lane - 1], F.gamma[(int64_t)f * K + lane - 1], qc, vc, wc);
        cz[lane] = -qc;
        ipos[lane] = F.parent_pos[(int64_t)f * K + lane - 1];
      }
    }
    for (int t = lane; t < p; t += kWave)
      if ((O >> t) & 1ull) oidx[mask_rank(O, t)] = t;
    __syncthreads();
    // V_OO and E_OO, V_OO + E_OO and the identity
    for (int idx = lane; idx < mo * mo; idx += kWave) {
      const int j = idx / mo, i = idx - j * mo;
      const int e = oidx[i] + oidx[j] * p;
      double v = 0.0;
      for (int k = 0; k < np; ++k) {
        double qc, vc, wc;
        lg_coefs<true>(M.model, alpha, F.length[(int64_t)f * K + k], F.gamma[(int64_t)f * K + k], qc, vc, wc);
        v += vc * R[(int64_t)F.color[(int64_t)f * K + k] * p * p + e];
      }
      const double en = lg_noise_E(Nz, sn, oidx[i], oidx[j], p, site);
      W1[i * ld + j] = v;
      W1[i * ld + mo + j] = en;
      W2[i * ld + j] = v + en;
      W2[i * ld + mo + j] = (i == j) ? 1.0 : 0.0;
    }
    // zt = z_O as the fill forms it, plus the displacement of the shifts
    for (int i = lane; i < mo; i += kWave) {
      const int t = oidx[i];
      double z = 0.0;
      for (int k = 0; k < np; ++k) {
        double qc, vc, wc;
        lg_coefs<true>(M.model, alpha, F.length[(int64_t)f * K + k], F.gamma[(int64_t)f * K + k], qc, vc, wc);
        if (theta) z += wc * theta[t];
        if (F.parent_pos[(int64_t)f * K + k] < 0) z += qc * mu[t];
      }
      z -= F.data[((int64_t)site * F.n_rows + F.data_row[f]) * p + t];
      z += lg_disp_d(S, Op, theta, alpha, F.length, F.gamma, f, K, np, t, p, site, 0);
      W1[i * ld + 2 * mo] = z;
      W2[i * ld + 2 * mo] = z;
    }
    __syncthreads();
    const double zi = (lane < mo) ? W1[lane * ld + 2 * mo] : 0.0;   // (mo <= 64: one lane per kept trait)
    double logdet_v, logdet_ve;
    if (!noise_gauss_jordan(W1, mo, nc, ld, lane, logdet_v)) { bad = true; break; }
    if (!noise_gauss_jordan(W2, mo, nc, ld, lane, logdet_ve)) { bad = true; break; }
    // D = -(j E)(j'), the upper triangle, into the left block of W1 (free since the elimination); D zt = -(j E)(j' zt) over
    // W1's last column (j zt is not needed)
    for (int idx = lane; idx < mo * mo; idx += kWave) {
      const int k = idx / mo, i = idx - k * mo;
      if (i > k) continue;
      double s = 0.0;
      for (int l = 0; l < mo; ++l) s += W1[i * ld + mo + l] * ((l <= k) ? W2[l * ld + mo + k] : W2[k * ld + mo + l]);
      W1[i * ld + k] = -s;
    }
    for (int i = lane; i < mo; i += kWave) {
      double s = 0.0;
      for (int l = 0; l < mo; ++l) s += W1[i * ld + mo + l] * W2[l * ld + 2 * mo];
      W1[i * ld + 2 * mo] = -s;
    }
    __syncthreads();
    // zt' D zt, lanes added by a fixed tree
    double q = (lane < mo) ? zi * W1[lane * ld + 2 * mo] : 0.0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
    // Delta J_ab += c_a c_b D (upper triangle mirrored: exactly symmetric), Delta h_a += c_a D zt at the kept traits of every
    // in-scope parent (the blocks of one family do not overlap)
    const int nn = np + 1;
    for (int idx = lane; idx < nn * nn * mo * mo; idx += kWave) {
      const int ab = idx / (mo * mo), ik = idx - ab * mo * mo;
      const int a = ab / nn, b = ab - a * nn;
      const int k = ik / mo, i = ik - k * mo;
      const int pa = ipos[a], pb = ipos[b];
      if (pa < 0 || pb < 0) continue;
      const unsigned long long ma = F.parent_mask ? F.parent_mask[(int64_t)f * K + a - 1] : full;
      const unsigned long long mb = F.parent_mask ? F.parent_mask[(int64_t)f * K + b - 1] : full;
      const double dv = (i <= k) ? W1[i * ld + k] : W1[k * ld + i];
      acc[(pa + mask_rank(ma, oidx[i])) + (pb + mask_rank(mb, oidx[k])) * m] += cz[a] * cz[b] * dv;
    }
    for (int idx = lane; idx < nn * mo; idx += kWave) {
      const int a = idx / mo, i = idx - a * mo;
      if (ipos[a] < 0) continue;
      const unsigned long long ma = F.parent_mask ? F.parent_mask[(int64_t)f * K + a - 1] : full;
      acc[m * m + ipos[a] + mask_rank(ma, oidx[i])] += cz[a] * W1[i * ld + 2 * mo];
    }
    if (lane == 0) acc[m * m + m] += -0.5 * (q + (logdet_ve - logdet_v));
  }
  __syncthreads();
  // the record, each entry by one lane: read what the fill wrote to the beliefs, write beliefs and factors
  const bool packed = bs && bs16::applies(m, fp);
  for (int idx = lane; idx < m * m; idx += kWave) {
    int o = idx;
    if (packed) {
      const int cc = idx / m, rr = idx - cc * m;
      if (!bs16::canonical(m, rr, cc, fp)) continue;
      o = bs16::J_off(m, rr, cc, fp);
    }
    const double v = out[o] + acc[idx];
    out[o] = v;
    if (fout) fout[o] = v;
  }
  for (int t = lane; t < m; t += kWave) {
    const int o = packed ? bs16::h_off(m, t, fp) : m * m + t;
    const double v = out[o] + acc[m * m + t];
    out[o] = v;
    if (fout) fout[o] = v;
  }
  if (lane == 0) {
    const int o = packed ? bs16::g_off(m, fp) : m * m + m;
    const double v = bad ? NAN : out[o] + acc[m * m + m];
    out[o] = v;
    if (fout) fout[o] = v;
  }
}

// The same for univariate batches in the site-minor layout (every belief dimension <= 2): thread = site, one row of
// workgroups per noisy cluster, closed-form scalars; per-site se2 comes from the [slot][site] copy, a line per wavefront.
__global__ __launch_bounds__(256) void noise_uni_sm_kernel(LgStatic F, LgParams M, LgShifts S, LgOptima Op, LgNoise Nz,
                                                           const int32_t* __restrict__ ncl, double* __restrict__ pool,
                                                           double* __restrict__ fpool, const int64_t* __restrict__ poff,
                                                           const int32_t* __restrict__ dim, int n_sites) {
  const int site = blockIdx.y * blockDim.x + threadIdx.x;
  if (site >= n_sites) return;
  const int c = ncl[blockIdx.x];
  const int64_t ns = sm_row(n_sites), ps = M.per_site ? site : 0;
  const int K = F.K;
  const double* __restrict__ R = M.R + ps * F.n_rates;
  const double mu = M.mu[ps];
  const double theta = M.theta ? M.theta[ps] : 0.0;
  const double alpha = (M.model == PGBP_LG_OU) ? M.alpha[ps] : 0.0;
  const double sig = Nz.sigma_e[Nz.per_site ? site : 0];
  const int m = dim[c];
  double J00 = 0, J10 = 0, J01 = 0, J11 = 0, h0 = 0, h1 = 0, g = 0;
  for (int fi = F.cl_off[c]; fi < F.cl_off[c + 1]; ++fi) {
    const int f = F.cl_fam[fi];
    const int sn = Nz.slot[f];
    if (sn < 0) continue;
    if (F.child_mask && !(F.child_mask[f] & 1ull)) continue;
    const int np = F.n_parents[f];
    double V = 0.0, z = 0.0;
    for (int k = 0; k < np; ++k) {
      double qc, vc, wc;
      lg_coefs<true>(M.model, alpha, F.length[(int64_t)f * K + k], F.gamma[(int64_t)f * K + k], qc, vc, wc);
      V += vc * R[F.color[(int64_t)f * K + k]];
      z += wc * theta;
      if (F.parent_pos[(int64_t)f * K + k] < 0) z += qc * mu;
      if (S.slot) {
        const int s = S.slot[(int64_t)f * K + k];
        if (s >= 0) z += F.gamma[(int64_t)f * K + k] * (S.per_site ? S.value_sm[(int64_t)s * ns + site] : S.value[s]);
      }
    }
    if (Op.regime) z += lg_optima_d(Op, &theta, alpha, F.length, F.gamma, f, K, np, 0, 1, site, ns);
    z -= F.data_sm[(int64_t)F.data_row[f] * ns + site];
    double E = Nz.scale[sn] * sig;
    if (Nz.se2) E += Nz.per_site ? Nz.se2_sm[(int64_t)sn * ns + site] : Nz.se2[sn];
    const double VE = V + E;
    const double D = -((1.0 / V) * E * (1.0 / VE));
    g += -0.5 * (z * D * z + (log(VE) - log(V)));
    if (!(VE > 0.0) || !(V > 0.0)) g = NAN;
    for (int a = 1; a <= np; ++a) {
      const int pa = F.parent_pos[(int64_t)f * K + a - 1];
      if (pa < 0) continue;
      double qa, vc, wc;
      lg_coefs<true>(M.model, alpha, F.length[(int64_t)f * K + a - 1], F.gamma[(int64_t)f * K + a - 1], qa, vc, wc);
      if (pa == 0) h0 += -qa * D * z; else h1 += -qa * D * z;
      for (int b = 1; b <= np; ++b) {
        const int pb = F.parent_pos[(int64_t)f * K + b - 1];
        if (pb < 0) continue;
        double qb;
        lg_coefs<true>(M.model, alpha, F.length[(int64_t)f * K + b - 1], F.gamma[(int64_t)f * K + b - 1], qb, vc, wc);
        const double v = qa * qb * D;
        if (pa == 0 && pb == 0) J00 += v;
        else if (pa == 1 && pb == 0) J10 += v;
        else if (pa == 0 && pb == 1) J01 += v;
        else J11 += v;
      }
    }
  }
  // [J (m*m) | h (m) | g] of the cluster, element t of site s at (poff + t) * ns + s
  const int64_t p0 = poff[c];
  double v[7];
  int len;
  if (m == 2) { v[0] = J00; v[1] = J10; v[2] = J01; v[3] = J11; v[4] = h0; v[5] = h1; v[6] = g; len = 7; }
  else if (m == 1) { v[0] = J00; v[1] = h0; v[2] = g; len = 3; }
  else { v[0] = g; len = 1; }
  for (int t = 0; t < len; ++t) {
    const int64_t o = (p0 + t) * ns + site;
    const double x = pool[o] + v[t];
    pool[o] = x;
    if (fpool) fpool[o] = x;
  }
}

void launch_lg_noise(const LgStatic& F, const LgParams& M, const LgShifts& S, const LgOptima& Op, const LgNoise& Nz,
                     const int32_t* d_ncl, int n_ncl,
                     double* pool, int64_t pool_stride, double* fpool, int64_t fpool_stride, const int64_t* d_boff,
                     const int32_t* d_dim, int bs16, int fast_p, int max_dim_ncl, int n_sites, hipStream_t st) {
  if (n_ncl <= 0 || !Nz.slot) return;
  LgOptima O = Op;
  O.value_sm = nullptr;   // (the [regime][site] rows are for lanes = sites)
  const int acc_cap = (int)noise_acc_cap(max_dim_ncl);
  const size_t bytes = lg_noise_lds_bytes(F.p, F.K, max_dim_ncl);   // (the engine has checked it against the compute unit's LDS)
  if (bytes > 64 * 1024) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(noise_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    (void)hipGetLastError();
  }
  hipLaunchKernelGGL(noise_kernel, dim3(n_ncl, n_sites), dim3(kWave), bytes, st, F, M, S, O, Nz, d_ncl, pool, pool_stride, fpool,
                     fpool_stride, d_boff, d_dim, bs16, fast_p, acc_cap);
}

void launch_lg_noise_uni_sm(const LgStatic& F, const LgParams& M, const LgShifts& S, const LgOptima& Op, const LgNoise& Nz,
                            const int32_t* d_ncl, int n_ncl, double* pool_sm, double* fpool_sm, const int64_t* d_poff, const int32_t* d_dim,
                            int n_sites, hipStream_t st) {
  if (n_ncl <= 0 || !Nz.slot) return;
  const int bs = n_sites >= 256 ? 256 : 64;
  hipLaunchKernelGGL(noise_uni_sm_kernel, dim3(n_ncl, (n_sites + bs - 1) / bs), dim3(bs), 0, st, F, M, S, Op, Nz, d_ncl, pool_sm,
                     fpool_sm, d_poff, d_dim, n_sites);
}

}  // namespace pgbp
