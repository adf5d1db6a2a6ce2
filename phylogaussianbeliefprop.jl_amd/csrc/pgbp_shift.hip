// Mean shifts on edges in the factor fill (pgbp_lg_set_shifts of include/pgbp.h): the reference's
// HeterogeneousShiftedBrownianMotion (src/evomodels/heterogeneousmodels.jl:152-179), whose factor code carries a
// displacement of the child's conditional mean through tree edges and hybrid nodes (src/evomodels/evomodels.jl:208-245,
// :314-330: the displacement of a hybrid is the gamma-weighted sum of its parent edges').
//
// A shift s_k on parent edge k of family f adds d = sum_k gamma_k s_k to the family's offset w (notation of pgbp_lgfill.hip),
// under BM and OU alike.  Variances, J and qc, vc, wc do not change; with O = child_mask[f], j = V_OO^-1, z = w - sum over the
// fixed nodes of c_a y_a as the fill forms it and delta = d_O, the family's factor changes by
//     Delta h_a = c_a j delta   at the kept traits of every in-scope node a (c_0 = 1, c_k = -qc_k),
//     Delta g   = -(delta' j z + delta' j delta / 2).
// The three fill kernels are left alone: these kernels run right after a fill whenever shifts are set and add the two terms
// to the records the fill wrote.  One workgroup (one wavefront) per (cluster that holds a shifted family, site) walks that
// cluster's families in table order, eliminates [V_OO | z | delta] in LDS, accumulates Delta h and Delta g of the cluster in
// LDS in family order and adds them to the record once: one writer per record, no atomics, every sum in a fixed order --
// the same bytes on every call.  Nothing is launched when no shift is set; the cost is that of the shifted clusters.
//
// Painted optima under OU (pgbp_lg_set_optima) enter here too: an edge of regime r displaces w by wc_k (theta_r - theta), so
// delta = (shifts' d + d_opt)_O (lg_disp_d of pgbp_shift_dev.hpp) and the clusters visited are those of either list.
#include <hip/hip_runtime.h>

#include "pgbp_bs16.hpp"
#include "pgbp_fam_dev.hpp"
#include "pgbp_kernels.hpp"
#include "pgbp_noise_dev.hpp"
#include "pgbp_shift_dev.hpp"

namespace pgbp {

extern __shared__ double shift_lds[];

// Gauss-Jordan on the n x nc system [V | z | delta] (row stride ld) in LDS by one wavefront: the right part becomes
// [V^-1 z | V^-1 delta]; false when a pivot is not positive (the fill made this cluster's g NaN already).
__device__ __forceinline__ bool shift_gauss_jordan(double* W, int n, int nc, int ld, int lane) {
  for (int k = 0; k < n; ++k) {
    const double d = W[k * ld + k];
    if (!(d > 0.0)) return false;
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
  return true;
}

// LDS of shift_kernel in doubles: Delta h (max_dim) and Delta g, the system, c_a, then the ints (positions, kept traits)
__host__ __device__ inline int shift_ld(int p) { return (p + 2) | 1; }
inline size_t shift_lds_doubles(int p, int K, int max_dim) {
  const size_t acc = ((size_t)max_dim + 1 + 1) & ~(size_t)1;
  return acc + (size_t)p * shift_ld(p) + (size_t)(K + 1) + (size_t)(K + 2 + p) / 2 + 2;
}

// plain and BS16 packed records.  shcl: the clusters that hold a shifted family; acc_cap: doubles kept for the accumulator
// OPT: the instance that also reads painted optima; without it the kernel is the shifts' own, as it was
template <bool OPT>
__global__ __launch_bounds__(64) void shift_kernel(LgStatic F, LgParams M, LgShifts S, LgOptima Op,
                                                   const int32_t* __restrict__ shcl,
                                                   double* __restrict__ pool, int64_t pool_stride, double* __restrict__ fpool,
                                                   int64_t fpool_stride, const int64_t* __restrict__ boff,
                                                   const int32_t* __restrict__ dim, int bs, int fp, int acc_cap) {
  const int lane = threadIdx.x, c = shcl[blockIdx.x], site = blockIdx.y;
  const int p = F.p, K = F.K;
  const int m = dim[c];
  double* __restrict__ out = pool + (int64_t)site * pool_stride + boff[c];
  double* __restrict__ fout = fpool ? fpool + (int64_t)site * fpool_stride + boff[c] : nullptr;
  double* dh = shift_lds;            // Delta h (m), Delta g at [m]
  double* W = shift_lds + acc_cap;   // mo x ld: [V_OO | z | delta]
  const int ldmax = shift_ld(p);
  double* cz = W + p * ldmax;        // c_a (K + 1)
  int* ipos = reinterpret_cast<int*>(cz + (K + 1));   // positions (K + 1), then the kept traits (p)
  int* oidx = ipos + (K + 1);
  for (int t = lane; t <= m; t += kWave) dh[t] = 0.0;
  const int64_t ps = M.per_site ? site : 0;
  const double* __restrict__ R = M.R + ps * F.n_rates * p * p;
  const double* __restrict__ mu = M.mu + ps * p;
  const double* __restrict__ theta = M.theta ? M.theta + ps * p : nullptr;
  const double alpha = (M.model == PGBP_LG_OU) ? M.alpha[ps] : 0.0;
  const unsigned long long full = p >= 64 ? ~0ull : ((1ull << p) - 1ull);
  bool bad = false;
  for (int fi = F.cl_off[c]; fi < F.cl_off[c + 1]; ++fi) {
    const int f = F.cl_fam[fi];
    const int np = F.n_parents[f];
    if (!lg_shift_any(S, f, K, np) && !(OPT && lg_optima_any(Op, f, K, np))) continue;   // (the same in every lane)
    const int cpos = F.child_pos[f];
    const unsigned long long O = F.child_mask ? (F.child_mask[f] & full) : full;
    const int mo = __popcll(O);
    if (mo == 0) continue;            // the factor is 1: a shift has nothing to displace
    const int nc = mo + 2, ld = nc | 1;
    __syncthreads();
    if (lane <= np) {
      if (lane == 0) {
        cz[0] = 1.0;
        ipos[0] = cpos;
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
    // V_OO
    for (int idx = lane; idx < mo * mo; idx += kWave) {
      const int j = idx / mo, i = idx - j * mo;
      const int e = oidx[i] + oidx[j] * p;
      double v = 0.0;
      for (int k = 0; k < np; ++k) {
        double qc, vc, wc;
        lg_coefs<true>(M.model, alpha, F.length[(int64_t)f * K + k], F.gamma[(int64_t)f * K + k], qc, vc, wc);
        v += vc * R[(int64_t)F.color[(int64_t)f * K + k] * p * p + e];
      }
      W[i * ld + j] = v;
    }
    // z_O as the fill forms it, and delta = d_O (a component of a shift outside O has no effect)
    for (int i = lane; i < mo; i += kWave) {
      const int t = oidx[i];
      double z = 0.0;
      for (int k = 0; k < np; ++k) {
        double qc, vc, wc;
        lg_coefs<true>(M.model, alpha, F.length[(int64_t)f * K + k], F.gamma[(int64_t)f * K + k], qc, vc, wc);
        if (theta) z += wc * theta[t];
        if (F.parent_pos[(int64_t)f * K + k] < 0) z += qc * mu[t];
      }
      if (cpos < 0) z -= F.data[((int64_t)site * F.n_rows + F.data_row[f]) * p + t];
      W[i * ld + mo] = z;
      W[i * ld + mo + 1] = OPT ? lg_disp_d(S, Op, theta, alpha, F.length, F.gamma, f, K, np, t, p, site, 0)
                               : lg_shift_d(S, F.gamma, f, K, np, t, p, site);
    }
    __syncthreads();
    const double di = (lane < mo) ? W[lane * ld + mo + 1] : 0.0;   // (mo <= 64: one lane per kept trait)
    if (!shift_gauss_jordan(W, mo, nc, ld, lane)) { bad = true; break; }
    // delta' j z + delta' j delta / 2, lanes added by a fixed tree
    double q = (lane < mo) ? di * (W[lane * ld + mo] + 0.5 * W[lane * ld + mo + 1]) : 0.0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
    // Delta h_a = c_a j delta at the kept traits of every in-scope node (the blocks of one family do not overlap)
    const int nn = np + 1;
    for (int idx = lane; idx < nn * mo; idx += kWave) {
      const int a = idx / mo, i = idx - a * mo;
      if (ipos[a] < 0) continue;
      const unsigned long long ma = (a == 0 || !F.parent_mask) ? (a == 0 ? O : full) : F.parent_mask[(int64_t)f * K + a - 1];
      dh[ipos[a] + mask_rank(ma, oidx[i])] += cz[a] * W[i * ld + mo + 1];
    }
    if (lane == 0) dh[m] += -q;
  }
  __syncthreads();
  // the record's h and g, each entry by one lane: read what the fill wrote to the beliefs, write beliefs and factors
  const bool packed = bs && bs16::applies(m, fp);
  for (int t = lane; t < m; t += kWave) {
    const int o = packed ? bs16::h_off(m, t, fp) : m * m + t;
    const double v = out[o] + dh[t];
    out[o] = v;
    if (fout) fout[o] = v;
  }
  if (lane == 0) {
    const int o = packed ? bs16::g_off(m, fp) : m * m + m;
    const double v = bad ? NAN : out[o] + dh[m];
    out[o] = v;
    if (fout) fout[o] = v;
  }
}

// The same for univariate batches in the site-minor layout (every belief dimension <= 2): thread = site, one row of
// workgroups per shifted cluster; the per-site values come from the [slot][site] copy, a line per wavefront.
template <bool OPT>
__global__ __launch_bounds__(256) void shift_uni_sm_kernel(LgStatic F, LgParams M, LgShifts S, LgOptima Op,
                                                           const int32_t* __restrict__ shcl, double* __restrict__ pool, double* __restrict__ fpool,
                                                           const int64_t* __restrict__ poff, const int32_t* __restrict__ dim,
                                                           int n_sites) {
  const int site = blockIdx.y * blockDim.x + threadIdx.x;
  if (site >= n_sites) return;
  const int c = shcl[blockIdx.x];
  const int64_t ns = sm_row(n_sites), ps = M.per_site ? site : 0;
  const int K = F.K;
  const double* __restrict__ R = M.R + ps * F.n_rates;
  const double mu = M.mu[ps];
  const double theta = M.theta ? M.theta[ps] : 0.0;
  const double alpha = (M.model == PGBP_LG_OU) ? M.alpha[ps] : 0.0;
  const int m = dim[c];
  double dh0 = 0, dh1 = 0, dg = 0;
  for (int fi = F.cl_off[c]; fi < F.cl_off[c + 1]; ++fi) {
    const int f = F.cl_fam[fi];
    const int np = F.n_parents[f], cpos = F.child_pos[f];
    if (!lg_shift_any(S, f, K, np) && !(OPT && lg_optima_any(Op, f, K, np))) continue;
    if (F.child_mask && !(F.child_mask[f] & 1ull)) continue;
    double V = 0.0, z = 0.0, d = 0.0;
    for (int k = 0; k < np; ++k) {
      double qc, vc, wc;
      lg_coefs<true>(M.model, alpha, F.length[(int64_t)f * K + k], F.gamma[(int64_t)f * K + k], qc, vc, wc);
      V += vc * R[F.color[(int64_t)f * K + k]];
      z += wc * theta;
      if (F.parent_pos[(int64_t)f * K + k] < 0) z += qc * mu;
      const int s = (!OPT || S.slot) ? S.slot[(int64_t)f * K + k] : -1;
      if (s >= 0) d += F.gamma[(int64_t)f * K + k] * (S.per_site ? S.value_sm[(int64_t)s * ns + site] : S.value[s]);
    }
    if (OPT && Op.regime) d += lg_optima_d(Op, &theta, alpha, F.length, F.gamma, f, K, np, 0, 1, site, ns);
    if (cpos < 0) z -= F.data_sm[(int64_t)F.data_row[f] * ns + site];
    const double j = 1.0 / V;
    dg += -(d * j * z + 0.5 * (d * j * d));
    for (int a = 0; a <= np; ++a) {
      const int pa = a == 0 ? cpos : F.parent_pos[(int64_t)f * K + a - 1];
      if (pa < 0) continue;
      double ca = 1.0;
      if (a > 0) {
        double qc, vc, wc;
        lg_coefs<true>(M.model, alpha, F.length[(int64_t)f * K + a - 1], F.gamma[(int64_t)f * K + a - 1], qc, vc, wc);
        ca = -qc;
      }
      if (pa == 0) dh0 += ca * j * d; else dh1 += ca * j * d;
    }
  }
  // [J (m*m) | h (m) | g] of the cluster, element t of site s at (poff + t) * ns + s
  const int64_t p0 = poff[c] + (int64_t)m * m;
  for (int t = 0; t <= m; ++t) {
    const int64_t o = (p0 + t) * ns + site;
    const double v = pool[o] + (t == m ? dg : (t == 0 ? dh0 : dh1));
    pool[o] = v;
    if (fpool) fpool[o] = v;
  }
}

// Per-site clade shifts of the optimum (pgbp_lg_set_clade_shifts_sites), on a thread-per-site engine in either layout: lanes =
// sites, a workgroup is 256 consecutive sites, grid.y runs over the clusters that hold a family inside some site's clade (the
// setter's list).  It runs after the shift and the noise corrections, so the factor of family f already stands at the offset
// z (shifts and painted optima included) and the variance V (+ E_f of a noisy tip); the clade's displacement
// delta = wc_f sum_j delta_j [f in clade(v_j)] (lg_clade_d) moves it by
//     Delta h_a = c_a j delta,   Delta g = -(delta j z + delta j delta / 2),   j = 1 / V,
// the statement of shift_uni_sm_kernel with the noisy variance.  A thread whose site has no slot covering a family of the
// cluster stores nothing; a record the per-site mask rewrites afterwards (pgbp_sitemiss.hip) is recomputed there with the same
// displacement.  One writer per record, no atomics, no barrier, contraction off, every sum in table order.
template <bool SM>
__global__ __launch_bounds__(256) void clade_shift_kernel(LgStatic F, LgParams M, LgShifts Sh, LgOptima Op, LgNoise Nz,
                                                          LgCladeShifts Cs, const int32_t* __restrict__ ccl,
                                                          double* __restrict__ pool, int64_t stride, double* __restrict__ fpool,
                                                          int64_t fstride, const int64_t* __restrict__ off,
                                                          const int32_t* __restrict__ dim, int n_sites) {
#pragma clang fp contract(off)
  const int site = blockIdx.x * 256 + threadIdx.x;
  if (site >= n_sites) return;   // (no barrier follows, and no other lane's store is this lane's to make)
  const int c = ccl[blockIdx.y];
  const int K = F.K;
  const int64_t ps = M.per_site ? site : 0;
  const double* __restrict__ R = M.R + ps * F.n_rates;
  const double mu = M.mu[ps], theta = M.theta ? M.theta[ps] : 0.0, alpha = M.alpha[ps];   // (launched under OU only)
  const int64_t drow = Cs.row;
  const int m = dim[c];
  double dh0 = 0.0, dh1 = 0.0, dg = 0.0;
  bool touched = false;
  for (int fi = F.cl_off[c]; fi < F.cl_off[c + 1]; ++fi) {
    const int f = F.cl_fam[fi];
    const int np = F.n_parents[f], cpos = F.child_pos[f];
    if (np == 0) continue;                                       // a root-prior family has no edge
    if (F.child_mask && !(F.child_mask[f] & 1ull)) continue;     // the factor is 1: nothing to displace
    bool any = false;
    const double d = lg_clade_d(Cs, alpha, F.length, F.gamma, f, K, np, site, any);
    if (!any) continue;
    touched = true;
    double V = 0.0, z = 0.0;
    for (int k = 0; k < np; ++k) {
      double qc, vc, wc;
      lg_coefs<true>(M.model, alpha, F.length[(int64_t)f * K + k], F.gamma[(int64_t)f * K + k], qc, vc, wc);
      V = V + vc * R[F.color[(int64_t)f * K + k]];
      z = z + wc * theta;
      if (F.parent_pos[(int64_t)f * K + k] < 0) z = z + qc * mu;   // the fixed root
    }
    z = z + lg_disp_d(Sh, Op, &theta, alpha, F.length, F.gamma, f, K, np, 0, 1, site, drow);
    if (cpos < 0) z = z - F.data_sm[(int64_t)F.data_row[f] * drow + site];   // a tip: its value
    const int sn = lg_noise_slot(Nz, f);
    if (sn >= 0) V = V + lg_noise_E(Nz, sn, 0, 0, 1, site);        // a noisy tip: V + E
    const double j = 1.0 / V;
    dg = dg + -((d * j) * z + 0.5 * ((d * j) * d));
    for (int a = 0; a <= np; ++a) {   // in-scope nodes: at most two
      const int pa = a == 0 ? cpos : F.parent_pos[(int64_t)f * K + a - 1];
      if (pa < 0) continue;
      double ca = 1.0, vc, wc;
      if (a > 0) {
        lg_coefs<true>(M.model, alpha, F.length[(int64_t)f * K + a - 1], F.gamma[(int64_t)f * K + a - 1], ca, vc, wc);
        ca = -ca;
      }
      if (pa == 0) dh0 = dh0 + (ca * j) * d;
      else dh1 = dh1 + (ca * j) * d;
    }
  }
  if (!touched) return;              // this (cluster, site) keeps the bytes it has
  // [J (m*m) | h (m) | g] of the cluster: element t of site s at (off + t) * stride + s, or at s * stride + off + t
  const int64_t o = off[c] + (int64_t)m * m;
  for (int t = 0; t <= m; ++t) {
    const double add = t == m ? dg : (t == 0 ? dh0 : dh1);
    const int64_t at = SM ? (o + t) * stride + site : (int64_t)site * stride + o + t;
    const double v = pool[at] + add;
    pool[at] = v;
    if (fpool) fpool[SM ? (o + t) * fstride + site : (int64_t)site * fstride + o + t] = v;
  }
}

void launch_lg_shift(const LgStatic& F, const LgParams& M, const LgShifts& S, const LgOptima& Op, const int32_t* d_shcl,
                     int n_shcl, double* pool,
                     int64_t pool_stride, double* fpool, int64_t fpool_stride, const int64_t* d_boff, const int32_t* d_dim,
                     int bs16, int fast_p, int max_dim, int n_sites, hipStream_t st) {
  if (n_shcl <= 0 || (!S.slot && !Op.regime)) return;
  LgOptima O = Op;
  O.value_sm = nullptr;   // (the [regime][site] rows are for lanes = sites)
  const int acc_cap = (max_dim + 1 + 1) & ~1;
  const size_t doubles = shift_lds_doubles(F.p, F.K, max_dim);
  const void* kern = O.regime ? reinterpret_cast<const void*>(shift_kernel<true>) : reinterpret_cast<const void*>(shift_kernel<false>);
  if (doubles * sizeof(double) > 64 * 1024) {
    (void)hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(doubles * sizeof(double)));
    (void)hipGetLastError();
  }
  if (O.regime)
    hipLaunchKernelGGL(shift_kernel<true>, dim3(n_shcl, n_sites), dim3(kWave), doubles * sizeof(double), st, F, M, S, O, d_shcl, pool,
                       pool_stride, fpool, fpool_stride, d_boff, d_dim, bs16, fast_p, acc_cap);
  else
    hipLaunchKernelGGL(shift_kernel<false>, dim3(n_shcl, n_sites), dim3(kWave), doubles * sizeof(double), st, F, M, S, O, d_shcl, pool,
                       pool_stride, fpool, fpool_stride, d_boff, d_dim, bs16, fast_p, acc_cap);
}

void launch_lg_shift_uni_sm(const LgStatic& F, const LgParams& M, const LgShifts& S, const LgOptima& Op, const int32_t* d_shcl,
                            int n_shcl,
                            double* pool_sm, double* fpool_sm, const int64_t* d_poff, const int32_t* d_dim, int n_sites,
                            hipStream_t st) {
  if (n_shcl <= 0 || (!S.slot && !Op.regime)) return;
  const int bs = n_sites >= 256 ? 256 : 64;
  if (Op.regime)
    hipLaunchKernelGGL(shift_uni_sm_kernel<true>, dim3(n_shcl, (n_sites + bs - 1) / bs), dim3(bs), 0, st, F, M, S, Op, d_shcl, pool_sm,
                       fpool_sm, d_poff, d_dim, n_sites);
  else
    hipLaunchKernelGGL(shift_uni_sm_kernel<false>, dim3(n_shcl, (n_sites + bs - 1) / bs), dim3(bs), 0, st, F, M, S, Op, d_shcl, pool_sm,
                       fpool_sm, d_poff, d_dim, n_sites);
}

void launch_lg_clade_shift(const LgStatic& F, const LgParams& M, const LgShifts& S, const LgOptima& Op, const LgNoise& Nz,
                           const LgCladeShifts& Cs, const int32_t* d_ccl, int n_ccl, int sm, double* pool, int64_t stride,
                           double* fpool, int64_t fstride, const int64_t* d_off, const int32_t* d_dim, int n_sites, hipStream_t st) {
  if (n_ccl <= 0 || !Cs.family) return;
  const int gx = (n_sites + 255) / 256;
  for (int c0 = 0; c0 < n_ccl; c0 += 65535) {   // (grid.y is 16 bits wide)
    const dim3 grid(gx, n_ccl - c0 < 65535 ? n_ccl - c0 : 65535);
    if (sm)
      hipLaunchKernelGGL(clade_shift_kernel<true>, grid, dim3(256), 0, st, F, M, S, Op, Nz, Cs, d_ccl + c0, pool, stride, fpool,
                         fstride, d_off, d_dim, n_sites);
    else
      hipLaunchKernelGGL(clade_shift_kernel<false>, grid, dim3(256), 0, st, F, M, S, Op, Nz, Cs, d_ccl + c0, pool, stride, fpool,
                         fstride, d_off, d_dim, n_sites);
  }
}

}  // namespace pgbp
