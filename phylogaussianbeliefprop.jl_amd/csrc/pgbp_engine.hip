// Device-resident ClusterGraphBelief + calibration driver behind the C ABI of include/pgbp.h.
// One engine = one HIP stream; every level of a traversal is one kernel launch on it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <limits>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

#include "pgbp_devmem.hpp"
#include "pgbp_internal.hpp"
#include "pgbp_kernels.hpp"
#include "pgbp_lgmodel.hpp"
#include "pgbp_sites_host.hpp"
#include "pgbp_topology.hpp"

using namespace pgbp;

namespace {

thread_local std::string g_create_error;  // (per thread: pgbp_group creates its engines concurrently)

// Kernel arguments in device memory: without it every launch of a narrow level pays a host-memory read for its
// 0x90-byte argument segment (measured: cfg3 +7 %, cfg5 +20 % per calibrate).  The HIP runtime reads the variable
// when it initialises, i.e. at the process's first HIP call; this constructor runs when the library is loaded
// (priority 101: ahead of the code object registration of this library), so a host that has not touched HIP yet --
// a Julia session that `dlopen`s libpgbp.so -- gets the setting without reading INTEGRATION.md.  A value the user
// exported is left alone; a host that initialised HIP earlier keeps whatever it had.
__attribute__((constructor(101))) void pgbp_default_environment() { setenv("HIP_FORCE_DEV_KERNARG", "1", 0); }

struct DevTraversal {
  DevBuf<int32_t> d_task_off;
  DevBuf<Entry> d_entries;
  DevBuf<URec> d_urecs;           // the entries as self-contained records (plans of univariate site batches: bp_level_uni1)
  DevBuf<FEntry> d_fentries;
  DevBuf<FPro> d_fpros;           // Traversal::fpros / cpros (null: no record of the traversal has a prologue)
  DevBuf<FPro> d_cpros;
  DevBuf<FEntry> d_centries;      // Traversal::centries: the groups of the chunks of fused levels
  DevBuf<int32_t> d_chunk_wg_off; // Traversal::chunk_wg_off
  DevBuf<int32_t> d_cgroups;      // Traversal::cgroups as first records of the tasks (Traversal::task_grec)
  DevBuf<int32_t> d_cgroups_task; // Traversal::cgroups as they are (task ids): the thread-per-site chunk kernel
  DevBuf<GRec> d_grecs;           // Traversal::grecs
  DevBuf<int32_t> d_rowmap;       // Traversal::rowmap
  // residual_kldiv! of sepsets beyond the LDS instance (kKlLdsMaxS): the entries concerned, ascending (device copy + host copy)
  DevBuf<int32_t> d_kl_big;
  std::vector<int32_t> kl_big;
};

// The engine's stream.  Declared ahead of every buffer of pgbp_engine, so that it is destroyed after all of them.
struct StreamOwner {
  hipStream_t s = nullptr;
  StreamOwner() = default;
  StreamOwner(const StreamOwner&) = delete;
  StreamOwner& operator=(const StreamOwner&) = delete;
  ~StreamOwner() { if (s) (void)hipStreamDestroy(s); }
  operator hipStream_t() const { return s; }
};

// Buffers that exist together or not at all: a set-up fills a local group and the engine takes it whole.
// the site-minor copies of the pools and the twins of the per-message / per-cluster word arrays
struct SmBufs {
  DevBuf<double> pool, fpool, rpool, kldiv;
  DevBuf<int32_t> flags, status, klflags, poison;
};
// pgbp_bm_tree; data_sm: [row][site] copy of data (p = 1, else null); ithl: [n_clusters] (1 / t, (p / 2) log t) of launch_bm_ithl
struct BmBufs {
  DevBuf<int32_t> kind, row;
  DevBuf<double> length, data, data_sm, Rinv, logdet, mu;
  DevBuf<double2> ithl;
};
// the levelled walk of pgbp_regularize_onschedule (OnSchedule)
struct OsBufs {
  DevBuf<int32_t> a_cl, ed_off, ed_msg, task_off;
  DevBuf<GRec> grecs;
  DevBuf<Entry> entries;
};

hipEvent_t hip_event(void* ev) { return static_cast<hipEvent_t>(ev); }

}  // namespace

// the two doors of pgbp_devmem.hpp to device memory, and the two to events
int pgbp::dev_malloc_bytes(void** p, size_t bytes) { return (int)hipMalloc(p, bytes); }
void pgbp::dev_free_bytes(void* p) { (void)hipFree(p); }
int pgbp::dev_event_create(void** ev) {
  hipEvent_t h = nullptr;
  const hipError_t rc = hipEventCreate(&h);
  *ev = rc == hipSuccess ? h : nullptr;
  return (int)rc;
}
void pgbp::dev_event_destroy(void* ev) { (void)hipEventDestroy(hip_event(ev)); }

struct pgbp_engine {
  Plan plan;
  StreamOwner st;   // (first: see StreamOwner)
  // the KL flags and divergences are as the last reset left them (nothing computed a KL residual since): the next reset of
  // the message flags leaves them alone (two of its three arrays; cfg4: 2.6 GB a call)
  bool kl_flags_clean = false, kl_div_clean = false;
  // device state
  DevBuf<double> d_pool;    // [n_sites][pool_stride] beliefs
  DevBuf<double> d_fpool;   // [n_sites][cluster_stride] factors
  DevBuf<double> d_rpool;   // [n_sites][rpool_stride] residuals
  DevBuf<MsgDesc> d_msgs;
  DevBuf<int32_t> d_idx;
  DevBuf<int32_t> d_flags;
  DevBuf<int32_t> d_status;
  DevBuf<double> d_kldiv;
  DevBuf<int32_t> d_klflags;     // [n_sites][n_msgs] iscalibrated_kl
  DevBuf<int32_t> d_nb_off;      // [n_clusters+1] -> d_nb_msg: the messages each cluster sends (regularisers)
  DevBuf<int32_t> d_nb_msg;
  DevBuf<int32_t> d_sepcl;       // [2*n_sepsets] sepset -> its two clusters
  DevBuf<double> d_eps;          // [n_sites][n_clusters] regularisation scratch
  DevBuf<double> d_thr;          // DevState::thr: residual-norm thresholds of the current tolerance
  DevBuf<double> d_logtab;       // DevState::logtab
  std::vector<double> h_thr;
  double thr_atol = 0.0;
  bool thr_valid = false;
  DevBuf<unsigned long long> d_fail;
  DevBuf<int32_t> d_poison;      // [n_sites][n_clusters]
  DevBuf<int32_t> d_iscal;       // [n_sites]
  DevBuf<int32_t> d_notcal;      // [n_sites] DevState::notcal
  DevBuf<int32_t> d_iscal_hist;  // [hist_cap][n_sites]
  int64_t hist_cap = 0;
  DevBuf<int64_t> d_boff;        // record offset tables for pack/unpack
  DevBuf<int64_t> d_packed_off;
  DevBuf<int64_t> d_roff;
  DevBuf<int64_t> d_rpacked_off;
  DevBuf<double> d_mu;    // [n_sites][max_dim]
  DevBuf<double> d_norm;  // [n_sites]
  DevBuf<int32_t> d_info; // [n_sites]
  DevBuf<int32_t> d_bdim;        // [n_beliefs] dims (layout conversion)
  DevBuf<int32_t> d_rdim;        // [n_msgs] sepset dim of every directed message
  DevBuf<int32_t> d_symflag;     // != 0: some precision matrix is not symmetric
  int32_t max_s = 0;                // largest sepset dimension
  // site-minor copies of the pools (univariate batches: every dimension <= 2), allocated at first use, and second copies of
  // the per-message / per-cluster word arrays: a layout switch transposes into them and swaps
  SmBufs sm;
  bool layout_sm = false;           // the live state is in the site-minor buffers
  bool layout_bs16 = false;         // current device layout of 16/32-dim beliefs and 16-dim residuals
  bool sym_known = false, sym_ok = false;
  // pgbp_regularize_onschedule: the levelled walk (OnSchedule) on the device, uploaded at its first call
  bool os_ready = false;
  OsBufs os;
  DevBuf<int32_t> d_one_task_off;  // single-message task for pgbp_propagate
  DevBuf<Entry> d_one_entry;
  DevBuf<GRec> d_one_rec;
  std::vector<DevTraversal> dpost, dpre;
  std::vector<DevBuf<FEntry>> d_tail;   // per tree: the tail groups of its postorder followed by those of its preorder
  std::vector<DevBuf<FPro>> d_tail_pros;  // ... and their prologues (null: none)
  // HIP events of the last pgbp_enqueue_calibrate_timed call (resolved by pgbp_fetch_kernel_time)
  std::vector<EventPair> kernel_events;
  int32_t kernel_launches = 0;
  DevBuf<double> d_ws;        // workspace of the kernels whose working matrix exceeds the LDS (beliefs above kLdsMaxDim)
  int64_t ws_cap = 0;
  DevBuf<double> d_gather;    // send slot of pgbp_comm_gather_loglik: [norm | info | succ, iscal]
  int64_t gather_cap = 0;
  DevBuf<double> d_xbuf;      // exchange buffer of pgbp_pack_beliefs / pgbp_unpack_beliefs
  int64_t xbuf_cap = 0;
  DevBuf<int64_t> d_xoff;     // ... its record offsets: [n] in the pool, [n + 1] in the buffer
  int64_t xoff_cap = 0;
  bool have_factors = false;
  // pgbp_bm_tree: static description + last parameters of the device factor fill
  bool bm_ready = false;
  int32_t bm_p = 0, bm_rows = 0, bm_per_site = 0;
  BmBufs bm;
  // pgbp_lg_setup: the linear-Gaussian model (table, device buffers, parameters, shifts, tip noise, topology); null: no table
  std::unique_ptr<LgModel> lg;
  std::string err;
  // a step of an asynchronous enqueue that could not be issued (a workspace that could not be allocated: ensure_ws has
  // set `err`): the launches that needed it were skipped; every entry point that enqueued, and the next pgbp_sync /
  // fetch, returns this code instead of results of messages that never ran
  int enqueue_rc = PGBP_OK;

  int fail(int code, const std::string& msg) {
    err = msg;
    return code;
  }
  int take_enqueue_rc() {
    const int rc = enqueue_rc;
    enqueue_rc = PGBP_OK;
    return rc;
  }
};

#define HIPCHK(e, call)                                                                          \
  do {                                                                                           \
    hipError_t _rc = (call);                                                                     \
    if (_rc != hipSuccess)                                                                       \
      return (e)->fail(PGBP_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(_rc));        \
  } while (0)

namespace {

// Every entry point makes its engine's device current first: a host that drives several engines on several devices (one
// host thread per engine: pgbp_group, pgbp_dist.hip) needs no hipSetDevice of its own.  The current device is per thread.
struct DeviceScope {
  explicit DeviceScope(const pgbp_engine* e) {
    if (e) (void)hipSetDevice(e->plan.device);
  }
};

// forget earlier failures: fail keys and the downstream-of-a-failure marks
int reset_fail(pgbp_engine* e);

template <class T>
int dev_alloc(pgbp_engine* e, DevBuf<T>& p, size_t n) {
  HIPCHK(e, hipError_t(p.alloc(n)));
  return PGBP_OK;
}

// `p` takes the new buffer only once the copy has succeeded: a failure leaves it as it was
template <class T>
int upload(pgbp_engine* e, DevBuf<T>& p, const std::vector<T>& v) {
  DevBuf<T> b;
  int rc = dev_alloc(e, b, v.size());
  if (rc) return rc;
  if (!v.empty()) HIPCHK(e, hipMemcpy(b.get(), v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  p = std::move(b);
  return PGBP_OK;
}

// the largest x with fl(x / c) <= atol (x -> fl(x / c) is monotone; IEEE division on the host = the device's)
double quotient_threshold(double c, double atol) {
  if (!(atol >= 0.0)) return -1.0;                 // NaN or negative tolerance: nothing passes (the maxima are >= 0)
  if (std::isinf(atol) || c == 0.0) return INFINITY;
  double x = atol * c;
  if (std::isinf(x)) x = std::numeric_limits<double>::max();
  while (x / c > atol) x = std::nextafter(x, -INFINITY);
  while (std::nextafter(x, INFINITY) / c <= atol) x = std::nextafter(x, INFINITY);
  return x;
}

// DevState::thr for the tolerance of this call (rebuilt and uploaded only when the tolerance changes)
int ensure_thresholds(pgbp_engine* e, double atol) {
  if (e->thr_valid && std::memcmp(&atol, &e->thr_atol, sizeof(double)) == 0) return PGBP_OK;
  HIPCHK(e, hipStreamSynchronize(e->st));   // (an earlier upload may still read the host copy)
  e->h_thr.assign(2 * (PGBP_MAX_DIM + 1), INFINITY);
  for (int s = 1; s <= PGBP_MAX_DIM; ++s) {
    e->h_thr[s] = quotient_threshold(std::sqrt((double)s), atol);
    e->h_thr[PGBP_MAX_DIM + 1 + s] = quotient_threshold(std::sqrt((double)s * (double)s), atol);
  }
  HIPCHK(e, hipMemcpyAsync(e->d_thr.get(), e->h_thr.data(), sizeof(double) * e->h_thr.size(), hipMemcpyHostToDevice, e->st));
  e->thr_atol = atol;
  e->thr_valid = true;
  return PGBP_OK;
}

DevState dev_state(pgbp_engine* e, const pgbp_opts* o) {
  DevState S;
  S.pool = e->d_pool.get();
  S.pool_stride = e->plan.pool_stride();
  S.rpool = e->d_rpool.get();
  S.rpool_stride = e->plan.rpool_stride();
  S.msgs = e->d_msgs.get();
  S.idx = e->d_idx.get();
  S.flags = e->d_flags.get();
  S.status = e->d_status.get();
  S.fail = e->d_fail.get();
  S.poison = e->d_poison.get();
  S.n_clusters = e->plan.n_clusters;
  S.n_msgs = e->plan.n_msgs();
  S.update_resnorm = o ? o->update_residualnorm : 1;
  S.atol = o ? o->atol : 1e-5;
  // (DevState::thr belongs to this tolerance: every entry point went through check_opts -> ensure_thresholds first)
  S.thr = e->d_thr.get();
  S.logtab = reinterpret_cast<const double2*>(e->d_logtab.get());
  const int sp = e->plan.fast_p > 0 ? e->plan.fast_p : 0;
  S.thr_h_p = e->h_thr.empty() ? 0.0 : e->h_thr[sp];
  S.thr_J_p = e->h_thr.empty() ? 0.0 : e->h_thr[PGBP_MAX_DIM + 1 + sp];
  S.bs16 = e->layout_bs16 ? 1 : 0;
  S.fast_p = e->plan.fast_p;
  S.sm = e->layout_sm ? 1 : 0;
  S.n_sites = e->plan.n_sites;
  S.packed_off = e->d_packed_off.get();
  S.rpacked_off = e->d_rpacked_off.get();
  S.sep_zero = 0;
  S.leaf_sepset = 0;
  S.notcal = nullptr;
  if (e->layout_sm) {
    S.pool = e->sm.pool.get();
    S.rpool = e->sm.rpool.get();
  }
  return S;
}

// The downstream-of-a-failure marks are one word per (site, cluster) -- 1.3 GB for cfg4's 8 000 problems x 40 000 clusters,
// a memset of it in front of every enqueue call was 3 % of a sharded step -- and a mark is only ever set beside a failure key
// in the site's fail word (the message that failed, or one downstream of it), which stays until the next reset_fail: so the
// marks are cleared only where some site's fail word holds a failure (every workgroup looks at the fail words first).
__global__ __launch_bounds__(256) void clear_poison_if_failed(const unsigned long long* __restrict__ fail, int n_sites,
                                                              int32_t* __restrict__ poison, int64_t n_words) {
  __shared__ int any;
  if (threadIdx.x == 0) any = 0;
  __syncthreads();
  for (int s = threadIdx.x; s < n_sites; s += blockDim.x)
    if (is_failure_key(fail[s])) any = 1;   // (every writer writes the same value)
  __syncthreads();
  if (!any) return;
  int4* p4 = reinterpret_cast<int4*>(poison);
  const int64_t n4 = n_words / 4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x)
    p4[i] = make_int4(0, 0, 0, 0);
  for (int64_t i = 4 * n4 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_words; i += (int64_t)gridDim.x * blockDim.x)
    poison[i] = 0;
}

// init_messagecalibrationflags_reset! on the device (src/clustergraphbeliefs.jl:190-202); reset_kl: the KL divergences too
void reset_message_flags(pgbp_engine* e, int reset_kl) {
  const int mode = ((reset_kl && !e->kl_div_clean) ? 1 : 0) | (e->kl_flags_clean ? 0 : 2);
  launch_reset_flags(e->d_msgs.get(), e->d_flags.get(), e->d_klflags.get(), e->d_kldiv.get(), e->plan.n_msgs(), e->plan.n_sites, mode, e->st,
                     e->layout_sm ? 1 : 0);
  e->kl_flags_clean = true;
  if (reset_kl) e->kl_div_clean = true;
}

int reset_fail(pgbp_engine* e) {
  const size_t ns = (size_t)e->plan.n_sites;
  // (either layout: the site-minor one has padded rows)
  const int64_t n_words = (int64_t)sm_row(e->plan.n_sites) * (int64_t)e->plan.n_clusters;
  const int64_t want = (n_words / 4 + 255) / 256;
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(want, 2048));
  hipLaunchKernelGGL(clear_poison_if_failed, dim3(grid), dim3(256), 0, e->st, e->d_fail.get(), (int)ns, e->d_poison.get(), n_words);
  HIPCHK(e, hipMemsetAsync(e->d_fail.get(), 0xFF, sizeof(unsigned long long) * ns, e->st));
  return PGBP_OK;
}

// Switch the device layout of every 16/32-dimensional belief (beliefs + factors) and every 16-dimensional
// residual between plain (ABI order, what the generic kernel and all transfers use) and BS16 (symmetric
// block-packed, what the register-resident kernel streams).  plain -> BS16 keeps the upper triangle, so it
// is only taken when every precision matrix is symmetric (checked once per upload).
// Site-minor layout of univariate batches (DevState::sm): the state moves between the plain pools and the site-minor
// buffers as a whole; only the traversals of bp_level_uni, the root integrate, reset-from-factors and the univariate
// factor fill work on the site-minor buffers, every other entry point asks for the plain layout first.
int ensure_site_minor(pgbp_engine* e, bool want) {
  const Plan& p = e->plan;
  if (want == e->layout_sm) return PGBP_OK;
  const size_t ns = (size_t)sm_row(p.n_sites);   // (rows of the site-minor buffers: padded)
  if (want && !e->sm.pool) {
    SmBufs B;
    int rc;
    if ((rc = dev_alloc(e, B.pool, ns * (size_t)p.packed_off.back()))) return rc;
    if ((rc = dev_alloc(e, B.fpool, ns * (size_t)p.packed_off[p.n_clusters]))) return rc;
    if ((rc = dev_alloc(e, B.rpool, ns * (size_t)p.rpacked_off.back()))) return rc;
    const size_t nm = (size_t)p.n_msgs();
    if ((rc = dev_alloc(e, B.flags, ns * nm))) return rc;
    if ((rc = dev_alloc(e, B.status, ns * nm))) return rc;
    if ((rc = dev_alloc(e, B.klflags, ns * nm))) return rc;
    if ((rc = dev_alloc(e, B.kldiv, ns * nm))) return rc;
    if ((rc = dev_alloc(e, B.poison, ns * (size_t)std::max(1, p.n_clusters)))) return rc;
    e->sm = std::move(B);
  }
  const int to = want ? 1 : 0;
  // flags, status, KL words and poison marks: [site][index] <-> [index][site]
  launch_transpose_words_i32(e->d_flags.get(), e->sm.flags.get(), p.n_msgs(), p.n_sites, to, e->st);
  launch_transpose_words_i32(e->d_status.get(), e->sm.status.get(), p.n_msgs(), p.n_sites, to, e->st);
  launch_transpose_words_i32(e->d_klflags.get(), e->sm.klflags.get(), p.n_msgs(), p.n_sites, to, e->st);
  launch_transpose_words_f64(e->d_kldiv.get(), e->sm.kldiv.get(), p.n_msgs(), p.n_sites, to, e->st);
  launch_transpose_words_i32(e->d_poison.get(), e->sm.poison.get(), p.n_clusters, p.n_sites, to, e->st);
  e->d_flags.swap(e->sm.flags);
  e->d_status.swap(e->sm.status);
  e->d_klflags.swap(e->sm.klflags);
  e->d_kldiv.swap(e->sm.kldiv);
  e->d_poison.swap(e->sm.poison);
  launch_site_minor(e->d_pool.get(), p.pool_stride(), e->sm.pool.get(), e->d_boff.get(), e->d_packed_off.get(), p.n_beliefs(), p.n_sites, to, e->st);
  launch_site_minor(e->d_fpool.get(), p.cluster_stride(), e->sm.fpool.get(), e->d_boff.get(), e->d_packed_off.get(), p.n_clusters, p.n_sites, to, e->st);
  launch_site_minor(e->d_rpool.get(), p.rpool_stride(), e->sm.rpool.get(), e->d_roff.get(), e->d_rpacked_off.get(), p.n_msgs(), p.n_sites, to, e->st);
  e->layout_sm = want;
  return PGBP_OK;
}

bool want_site_minor(const pgbp_engine* e) {
  return e->plan.tune.packed_layouts && e->plan.max_dim <= 2 && e->plan.n_sites >= 64;
}

// many tiny problems (every belief <= 2 variables, at least 8 sites): every task of a traversal runs on the thread-per-site
// kernels (bp_level_uni / uni1, lanes = sites), whatever class the planner gave it
bool uni_engine(const pgbp_engine* e) { return e->plan.max_dim <= 2 && e->plan.n_sites >= 8; }

static int ensure_bs16(pgbp_engine* e, bool want_bs16);

// The BS16 conversion works on the plain pools: the site-minor layout is left before it and entered after it, and excludes
// BS16 (its buffers hold plain records, element by element).
int ensure_layout(pgbp_engine* e, bool want_bs16, bool want_sm = false) {
  int rc;
  if (want_sm) want_bs16 = false;
  if (e->layout_sm && !want_sm && (rc = ensure_site_minor(e, false))) return rc;
  if ((rc = ensure_bs16(e, want_bs16))) return rc;
  if (want_sm && !e->layout_sm && (rc = ensure_site_minor(e, true))) return rc;
  return PGBP_OK;
}

static int ensure_bs16(pgbp_engine* e, bool want_bs16) {
  const Plan& p = e->plan;
  if (want_bs16 == e->layout_bs16) return PGBP_OK;
  if (want_bs16) {
    if (!e->sym_known) {
      HIPCHK(e, hipMemsetAsync(e->d_symflag.get(), 0, sizeof(int32_t), e->st));
      launch_check_symmetry(e->d_pool.get(), p.pool_stride(), e->d_boff.get(), e->d_bdim.get(), p.n_beliefs(), p.n_sites, e->d_symflag.get(), p.fast_p, e->st);
      launch_check_symmetry(e->d_fpool.get(), p.cluster_stride(), e->d_boff.get(), e->d_bdim.get(), p.n_clusters, p.n_sites, e->d_symflag.get(), p.fast_p, e->st);
      int32_t flag = 0;
      HIPCHK(e, hipMemcpyAsync(&flag, e->d_symflag.get(), sizeof(flag), hipMemcpyDeviceToHost, e->st));
      HIPCHK(e, hipStreamSynchronize(e->st));
      e->sym_known = true;
      e->sym_ok = flag == 0;
    }
    if (!e->sym_ok) return PGBP_OK;  // stay plain: exact reference semantics for asymmetric input
  }
  const int to = want_bs16 ? 1 : 0;
  launch_convert_layout(e->d_pool.get(), p.pool_stride(), e->d_boff.get(), e->d_bdim.get(), p.n_beliefs(), p.n_sites, to, 0, p.fast_p, e->st);
  launch_convert_layout(e->d_fpool.get(), p.cluster_stride(), e->d_boff.get(), e->d_bdim.get(), p.n_clusters, p.n_sites, to, 0, p.fast_p, e->st);
  launch_convert_layout(e->d_rpool.get(), p.rpool_stride(), e->d_roff.get(), e->d_rdim.get(), p.n_msgs(), p.n_sites, to, 1, p.fast_p, e->st);
  e->layout_bs16 = want_bs16;
  return PGBP_OK;
}

// layout wanted by the traversals of the current schedule
// The postorder of tree 0 writes every sepset and, straight after a reset, would read only zeros from them: true when
// that traversal runs entirely on kernels that honour DevState::sep_zero (the register-resident ones; the thread-per-site
// ones of the site-minor layout) and the schedule tree spans every sepset (a clique tree, the Bethe graph of a tree).
bool fresh_sepsets_shortcut(const pgbp_engine* e) {
  const Plan& p = e->plan;
  // (the site-minor layout belongs to the thread-per-site kernels, which honour it too)
  return (e->layout_sm || p.all_fast) && !p.trees.empty() && (int)p.trees[0].pa.size() == p.n_sepsets;
}

bool want_bs16(const pgbp_engine* e) {
  // (packed tiles: even P; not for the thread-per-site engines, whose kernels read plain records -- a clique tree whose
  // sepsets all hold 2 variables is all fast-class with P = 2)
  return e->plan.tune.packed_layouts && e->plan.all_fast && e->plan.fast_p > 0 && e->plan.fast_p % 2 == 0 && !uni_engine(e);
}

void free_traversals(pgbp_engine* e) {
  e->dpost.clear();
  e->dpre.clear();
  e->d_tail.clear();
  e->d_tail_pros.clear();
}

// at least `doubles` of workspace (grown when a launch needs more: the stream is drained first, kernels in flight use it)
int ensure_ws(pgbp_engine* e, int64_t doubles) {
  if (doubles <= e->ws_cap) return PGBP_OK;
  HIPCHK(e, hipStreamSynchronize(e->st));
  e->ws_cap = 0;
  const int rc = dev_alloc(e, e->d_ws, (size_t)doubles);
  if (rc) return rc;
  e->ws_cap = doubles;
  return PGBP_OK;
}

// Every entry point that launches a message kernel comes through here BEFORE its first launch: the options are sane and
// the threshold table of DevState::thr is the one of this tolerance (a failed upload is this call's error, not a launch
// with whatever the table held).
int check_opts(pgbp_engine* e, const pgbp_opts* o) {
  if (o && !(o->atol >= 0.0)) return e->fail(PGBP_ERR_INVALID, "pgbp_opts.atol must be >= 0");
  const int rc = ensure_thresholds(e, o ? o->atol : 1e-5);
  if (rc != PGBP_OK) e->thr_valid = false;
  return rc;
}

unsigned long long seq_stride(const pgbp_engine* e) {
  size_t mx = 0;
  for (const Tree& t : e->plan.trees) mx = std::max(mx, t.pa.size());
  return 2ull * (mx + 1);
}

// how many levels at the root end of a traversal the tail launch takes over (0: none)
int tail_levels(const pgbp_engine* e, const Traversal& tr, bool kl) {
  // residual_kldiv! runs between levels; the site-minor layout belongs to the thread-per-site kernel
  if (kl || e->layout_sm || uni_engine(e) || !e->plan.tune.tail) return 0;
  return tr.tail_levels;
}

// a loop launch (the tail, a chunk of fused levels): pgbp_loop.hip in the packed layout, pgbp_fast.hip's loop mode otherwise
void launch_loop_or_tail(pgbp_engine* e, const DevState& S, const FEntry* recs, const FPro* pros, int ngroups, int split,
                         unsigned long long seq_base, unsigned long long stop_a, unsigned long long stop_b,
                         const int32_t* d_wg_off, int n_wg) {
  if (e->plan.tune.loop2 && S.bs16 && e->plan.fast_p % 2 == 0)
    launch_loop16(S, recs, pros, ngroups, split, e->plan.n_sites, seq_base, stop_a, stop_b, e->st, d_wg_off, n_wg);
  else
    launch_fast16(S, recs, pros, kFastTail, ngroups, split, e->plan.n_sites, seq_base, stop_a, stop_b, e->st, d_wg_off, n_wg);
}

// levels [L0, L1) of one traversal: one launch per level (two where a level mixes fast-class and generic tasks)
void enqueue_levels(pgbp_engine* e, const DevState& S, const Traversal& tr, const DevTraversal& d, int L0, int L1,
                    unsigned long long seq_base, unsigned long long stop_below, bool kl, int* launches) {
  const bool uni = uni_engine(e);  // many tiny problems: lanes = sites (bp_level_uni / uni1)
  // (the loop mode of the thread-per-site kernels exists for sepsets of at most one variable: bp_chunk_uni1)
  const bool chunks_on = !kl && e->plan.tune.tail && (uni ? e->max_s <= 1 : !e->layout_sm);
  size_t next_chunk = 0;
  for (int L = L0; L < L1; ++L) {
    if (chunks_on) {
      // a chunk of fused levels starting here (and ending inside the range): one launch, one workgroup per tree of tasks
      while (next_chunk < tr.chunks.size() && tr.chunks[next_chunk].level0 < L) ++next_chunk;
      if (next_chunk < tr.chunks.size() && tr.chunks[next_chunk].level0 == L && tr.chunks[next_chunk].level1 <= L1) {
        const Traversal::Chunk& ch = tr.chunks[next_chunk];
        if (uni && d.d_urecs.get())   // (the planner builds chunks of tasks for such plans: pgbp_plan.cpp, plan_uni)
          launch_chunk_uni1(S, d.d_task_off.get(), d.d_urecs.get(), d.d_cgroups_task.get() + ch.group0 * kTailWaves, d.d_chunk_wg_off.get() + ch.wg0,
                            ch.n_wg, e->plan.n_sites, seq_base, stop_below, e->st);
        else if (ch.generic)
          launch_chunk_generic(S, d.d_grecs.get(), d.d_cgroups.get() + ch.group0 * kTailWaves, d.d_chunk_wg_off.get() + ch.wg0, ch.n_wg,
                               e->plan.n_sites, seq_base, stop_below, ch.max_mf, ch.small_only != 0, e->plan.tune.pair2, e->st);
        else
          launch_loop_or_tail(e, S, d.d_centries.get() + ch.group0 * kTailWaves, d.d_cpros.get() ? d.d_cpros.get() + ch.group0 * kTailWaves : nullptr,
                              ch.n_groups, INT32_MAX, seq_base, stop_below, stop_below, d.d_chunk_wg_off.get() + ch.wg0, ch.n_wg);
        if (launches) *launches += 1;
        L = ch.level1 - 1;
        continue;
      }
    }
    const int t0 = tr.level_off[L], nt = tr.level_off[L + 1] - t0;
    // (a thread-per-site engine: the level's fast-class tasks too -- with 2-variable sepsets the planner finds some, and the
    // register-resident kernel knows nothing of the site-minor layout)
    const int nf = uni ? 0 : tr.level_nfast[L], ng = uni ? 0 : tr.level_ngroups[L];
    launch_fast16(S, d.d_fentries.get() + tr.level_fbase[L], d.d_fpros.get() ? d.d_fpros.get() + tr.level_fbase[L] : nullptr, kFastLevel, ng, ng,
                  e->plan.n_sites, seq_base, stop_below, stop_below, e->st);
    const int nbig = tr.level_nbig[L];
    if (uni)
      launch_level_uni(S, d.d_task_off.get(), d.d_entries.get(), d.d_urecs.get(), t0, nt, e->plan.n_sites, seq_base, stop_below, e->max_s, e->st);
    else {
      const bool rows = d.d_rowmap.get() && !tr.level_nrows.empty() && tr.level_nrows[L] > 0;
      launch_level_generic(S, d.d_grecs.get(), tr.level_gbase[L], nt - nf - nbig, e->plan.n_sites, seq_base, stop_below,
                           tr.max_mf, nbig == 0 && tr.level_small[L] != 0, e->st,
                           rows ? d.d_rowmap.get() + 2 * tr.level_rowbase[L] : nullptr, rows ? tr.level_nrows[L] : 0,
                           e->plan.tune.small4_min);
      if (nbig > 0) {
        if (ensure_ws(e, (int64_t)nbig * e->plan.n_sites * big_ws_doubles(tr.max_mf_big)) == PGBP_OK)
          launch_level_big(S, d.d_task_off.get(), d.d_entries.get(), t0 + nt - nbig, nbig, e->plan.n_sites, seq_base, stop_below,
                           tr.max_mf_big, e->d_ws.get(), e->st);
        else
          e->enqueue_rc = PGBP_ERR_HIP;   // (these messages never ran: the entry point reports it)
      }
    }
    if (launches) *launches += (nf > 0) + (nt - nf - nbig > 0) + (nbig > 0);
    if (kl) {  // residual_kldiv! right after the messages of the level (src/calibration.jl:128,154)
      const int e0 = tr.task_off[t0], e1 = tr.task_off[t0 + nt];
      int level_s = 0;   // the largest sepset of THIS level's messages sizes the launch's LDS, not the graph's largest
      for (int q = e0; q < e1; ++q) level_s = std::max(level_s, (int)e->plan.msgs[tr.entries[q].msg].s);
      // the level's entries whose sepset is beyond the LDS instance: a second launch with a workspace slab each
      const auto b0 = std::lower_bound(d.kl_big.begin(), d.kl_big.end(), e0), b1 = std::lower_bound(d.kl_big.begin(), d.kl_big.end(), e1);
      const int n_big = (int)(b1 - b0);
      e->kl_flags_clean = e->kl_div_clean = false;
      if (n_big == 0 || ensure_ws(e, (int64_t)n_big * e->plan.n_sites * kldiv_ws_doubles(level_s)) == PGBP_OK)
        launch_residual_kldiv(S, d.d_entries.get(), e0, e1 - e0, level_s, e->d_kldiv.get(), e->d_klflags.get(), e->plan.n_sites, stop_below, e->st,
                              d.d_kl_big.get() + (b0 - d.kl_big.begin()), n_big, e->d_ws.get());
      else
        e->enqueue_rc = PGBP_ERR_HIP;
    }
  }
}

// Traversals of one schedule tree.  dirs: 1 = postorder only, 2 = preorder only, 3 = postorder then preorder (one
// iteration of calibrate! on this tree: src/calibration.jl:72-84).  The narrow levels at the root end of the tree go out
// as ONE single-workgroup launch (Traversal::tail_levels); in a postorder + preorder pair the postorder's last levels and
// the preorder's first ones share it.
// Once the postorder of a tree failed, its preorder does not run here.  (The reference still walks it, on beliefs the
// sequential postorder left half-updated, may log a second failure, and returns (false, false): src/calibration.jl:80-82.
// The first failure of the reference's order is what the engine reports; the state after a failure is unspecified.)
void enqueue_tree(pgbp_engine* e, const DevState& S_in, int tree, int dirs, unsigned long long pair_index, bool kl = false,
                  int* n_launches = nullptr) {
  const Tree& T = e->plan.trees[tree];
  const unsigned long long seq_base = pair_index * seq_stride(e);
  const unsigned long long stop_post = seq_base, stop_pre = seq_base + (unsigned long long)T.pa.size();
  // LEAF SEPSETS (FEntry::pad[3]): only when this very call runs the postorder that fills them in front of the preorder that
  // would read them, and every message of it runs on the register-resident kernels (they copy a leaf's belief into its
  // sepset bit for bit; kl: residual_kldiv! reads the sepsets between the levels, on the generic path's terms)
  DevState S = S_in;
  S.leaf_sepset = (dirs == 3 && !kl && e->plan.tune.leaf_sepset && e->plan.all_fast && !uni_engine(e) && !e->layout_sm) ? 1 : 0;
  const int np = (dirs & 1) ? tail_levels(e, T.post, kl) : 0, nq = (dirs & 2) ? tail_levels(e, T.pre, kl) : 0;
  const int nlev_post = (int)T.post.level_off.size() - 1, nlev_pre = (int)T.pre.level_off.size() - 1;
  if (dirs & 1) enqueue_levels(e, S, T.post, e->dpost[tree], 0, nlev_post - np, seq_base, stop_post, kl, n_launches);
  if (np + nq > 0) {
    // d_tail = the postorder's tail groups followed by the preorder's
    const size_t first = (size_t)(np > 0 ? 0 : T.post.tail_levels) * kTailWaves;
    launch_loop_or_tail(e, S, e->d_tail[tree].get() + first, e->d_tail_pros[tree] ? e->d_tail_pros[tree].get() + first : nullptr, np + nq,
                        np, seq_base, stop_post, stop_pre, nullptr, 0);
    if (n_launches) *n_launches += 1;
  }
  if (dirs & 2) enqueue_levels(e, S, T.pre, e->dpre[tree], nq, nlev_pre, seq_base, stop_pre, kl, n_launches);
}

// One iteration of calibrate! on one schedule tree (postorder + preorder) followed by iscalibrated_residnorm(beliefs) into
// `d_out` [n_sites].  Thread-per-site engines whose tree holds every sepset: the message kernels mark the sites with a false
// flag themselves (DevState::notcal) and the all-flags reduction is a kernel of n_sites threads instead of one over
// n_sites x n_messages words.  Engines whose every message runs on the register-resident kernels (bp_fast16, bp_loop16) do
// the same: one launch of n_sites workgroups in place of the fill of `d_out` and the reduction.
void enqueue_pair_and_iscal(pgbp_engine* e, const DevState& S, int tree, unsigned long long pair, bool kl, int32_t* d_out,
                            int* n_launches = nullptr) {
  const Plan& p = e->plan;
  const bool fused = e->layout_sm && !kl && S.update_resnorm != 0 && (int)p.trees[tree].pa.size() == p.n_sepsets;
  // (not for a tree with prologues: the loop kernel's prologue instance sets no marks, pgbp_loop.hip; nor on the lane grids
  // whose instances set none: leaf_mark_grid)
  const bool fused_fast = !fused && leaf_mark_grid(p.fast_p + (p.fast_p & 1)) && !e->layout_sm && !uni_engine(e) && p.all_fast && !kl && S.update_resnorm != 0 &&
                          (int)p.trees[tree].pa.size() == p.n_sepsets && !p.trees[tree].post.has_pro && !p.trees[tree].pre.has_pro;
  if (fused) {
    (void)hipMemsetAsync(e->d_notcal.get(), 0, sizeof(int32_t) * (size_t)p.n_sites, e->st);
    DevState S1 = S;
    S1.notcal = e->d_notcal.get();
    enqueue_tree(e, S1, tree, 3, pair, kl, n_launches);
    launch_iscal_from_notcal(e->d_notcal.get(), d_out, p.n_sites, e->st);
  } else if (fused_fast) {
    // the register-resident kernels mark a false flag too.  A message that failed or did not run (behind a failure, at a
    // site `auto` has halted) leaves its flag as it was, and that flag counts: such a site -- its fail word holds a key
    // below the end of this pair -- gets the reduction over its flags inside the same launch.  That launch also clears the
    // marks it has read: no fill in front of the traversals (d_notcal is clear from pgbp_create on).
    DevState S1 = S;
    S1.notcal = e->d_notcal.get();
    enqueue_tree(e, S1, tree, 3, pair, kl, n_launches);
    launch_iscal_from_notcal_or_flags(e->d_notcal.get(), e->d_flags.get(), p.n_msgs(), e->d_fail.get(), (pair + 1) * seq_stride(e), d_out,
                                      p.n_sites, e->st);
  } else {
    enqueue_tree(e, S, tree, 3, pair, kl, n_launches);
    launch_reduce_flags(e->d_flags.get(), p.n_msgs(), p.n_sites, d_out, e->st, e->layout_sm ? 1 : 0);
  }
}

// integratebelief! of one belief in whatever layout the state is in
void integrate_async(pgbp_engine* e, int belief, double* d_mu) {
  const Plan& p = e->plan;
  if (e->layout_sm)
    launch_integrate_sm(e->sm.pool.get(), p.packed_off[belief], p.dims[belief], d_mu, std::max(1, p.max_dim), e->d_norm.get(),
                        e->d_info.get(), p.n_sites, e->st);
  else if (ensure_ws(e, (int64_t)p.n_sites * big_ws_doubles(p.dims[belief])) == PGBP_OK)
    launch_integrate(e->d_pool.get(), p.pool_stride(), p.boff[belief], p.dims[belief], e->layout_bs16 ? 1 : 0, p.fast_p, d_mu,
                     std::max(1, p.max_dim), e->d_norm.get(), e->d_info.get(), p.n_sites, e->d_ws.get(), e->st);
  else
    e->enqueue_rc = PGBP_ERR_HIP;   // (e->err is set; the entry point returns the code)
}

// skip_sepsets: the caller's next traversal overwrites every sepset without reading it (DevState::sep_zero)
int reset_from_factors_async(pgbp_engine* e, bool skip_sepsets = false) {
  if (!e->have_factors) return e->fail(PGBP_ERR_STATE, "no factors: call pgbp_set_beliefs(snapshot) or pgbp_init_factors_frombeliefs first");
  const Plan& p = e->plan;
  if (e->layout_sm) {  // cluster elements come first and are contiguous over sites
    const int64_t nc = p.packed_off[p.n_clusters] * sm_row(p.n_sites), nall = p.packed_off.back() * sm_row(p.n_sites);
    HIPCHK(e, hipMemcpyAsync(e->sm.pool.get(), e->sm.fpool.get(), sizeof(double) * (size_t)nc, hipMemcpyDeviceToDevice, e->st));
    if (!skip_sepsets) HIPCHK(e, hipMemsetAsync(e->sm.pool.get() + nc, 0, sizeof(double) * (size_t)(nall - nc), e->st));
    return PGBP_OK;
  }
  if (e->layout_bs16)  // packed records use about half of their slots: copy what is in use
    launch_copy_records(e->d_fpool.get(), p.cluster_stride(), e->d_pool.get(), p.pool_stride(), e->d_boff.get(), e->d_bdim.get(), p.n_clusters, 1,
                        p.fast_p, p.n_sites, e->st);
  else
    launch_copy_strided(e->d_fpool.get(), p.cluster_stride(), e->d_pool.get(), p.pool_stride(), p.cluster_stride(), p.n_sites, e->st);
  if (!skip_sepsets)
    launch_zero_strided(e->d_pool.get() + p.cluster_stride(), p.pool_stride(), p.pool_stride() - p.cluster_stride(),
                        p.n_sites, e->st);
  return PGBP_OK;
}

void decode_fail(const pgbp_engine* e, unsigned long long key, pgbp_result& r) {
  const unsigned long long q = key >> kInfoBits;
  r.fail_info = (int32_t)(key & ((1ull << kInfoBits) - 1));
  const unsigned long long stride = seq_stride(e);
  const unsigned long long pair = q / stride, seq = q % stride;
  const int nt = (int)e->plan.trees.size();
  r.fail_iter = (int32_t)(pair / nt) + 1;
  r.fail_tree = (int32_t)(pair % nt) + 1;
  const int n = (int)e->plan.trees[pair % nt].pa.size();
  if ((int)seq < n) {
    r.fail_dir = 0;
    r.fail_edge = n - 1 - (int)seq;
  } else {
    r.fail_dir = 1;
    r.fail_edge = (int)seq - n;
  }
}

}  // namespace

extern "C" {

const char* pgbp_last_error(const pgbp_engine* e) { return e ? e->err.c_str() : g_create_error.c_str(); }

void pgbp_destroy(pgbp_engine* e) {
  if (!e) return;
  (void)hipSetDevice(e->plan.device);
  delete e;   // (the first release waits for the device, as hipFree does; the buffers go before the stream)
}

int pgbp_create(const pgbp_desc* desc, pgbp_engine** out) {
  if (!out) return PGBP_ERR_INVALID;
  *out = nullptr;
  std::unique_ptr<pgbp_engine> up(new pgbp_engine());
  pgbp_engine* e = up.get();
  int rc = plan_build(e->plan, desc);
  if (rc) {
    g_create_error = e->plan.err;
    return rc;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || desc->device < 0 || desc->device >= ndev) {
    g_create_error = "no usable HIP device (device " + std::to_string(desc->device) + " of " + std::to_string(ndev) +
                     "): the engine has no CPU path";
    return PGBP_ERR_NO_DEVICE;
  }
  auto bail = [&](int code) {
    g_create_error = e->err;
    pgbp_destroy(up.release());
    return code;
  };
  if (hipSetDevice(desc->device) != hipSuccess) {
    e->err = "hipSetDevice failed";
    return bail(PGBP_ERR_HIP);
  }
  if (hipStreamCreateWithFlags(&e->st.s, hipStreamNonBlocking) != hipSuccess) {
    e->err = "hipStreamCreate failed";
    return bail(PGBP_ERR_HIP);
  }
  const Plan& p = e->plan;
  const size_t ns = (size_t)p.n_sites;
  const size_t nm = (size_t)p.n_msgs();
  const size_t nsw = (size_t)sm_row(p.n_sites);   // the per-message / per-cluster word arrays serve both layouts (a switch swaps
                                                   // them with their twins): sized for the padded rows of the site-minor one
  // (kPoolTail: the loop-launch kernel issues every sender load whatever the record is; for a constant's one-double record
  // the right-hand planes of a packed tile lie up to 130 doubles behind its start -- past the end of the last site's pool if
  // little follows it there.  The values are ignored; the addresses must be valid.)
  constexpr size_t kPoolTail = 256;
  if ((rc = dev_alloc(e, e->d_pool, ns * p.pool_stride() + kPoolTail))) return bail(rc);
  if ((rc = dev_alloc(e, e->d_fpool, ns * p.cluster_stride()))) return bail(rc);
  if ((rc = dev_alloc(e, e->d_rpool, ns * p.rpool_stride()))) return bail(rc);
  if ((rc = upload(e, e->d_msgs, p.msgs))) return bail(rc);
  if ((rc = upload(e, e->d_idx, p.idxpool))) return bail(rc);
  if ((rc = dev_alloc(e, e->d_flags, nsw * nm))) return bail(rc);
  if ((rc = dev_alloc(e, e->d_status, nsw * nm))) return bail(rc);
  if ((rc = dev_alloc(e, e->d_kldiv, nsw * nm))) return bail(rc);
  if ((rc = dev_alloc(e, e->d_klflags, nsw * nm))) return bail(rc);
  {
    std::vector<int32_t> nb_off(p.n_clusters + 1, 0), nb_msg(nm);
    for (int k = 0; k < p.n_sepsets; ++k) {
      ++nb_off[p.sepset_clusters[2 * k] + 1];
      ++nb_off[p.sepset_clusters[2 * k + 1] + 1];
    }
    for (int c = 0; c < p.n_clusters; ++c) nb_off[c + 1] += nb_off[c];
    std::vector<int32_t> fill(nb_off.begin(), nb_off.end() - 1);
    for (int k = 0; k < p.n_sepsets; ++k) {  // message 2k is received by cluster a (sent by b), 2k+1 the reverse
      nb_msg[fill[p.sepset_clusters[2 * k]]++] = 2 * k + 1;
      nb_msg[fill[p.sepset_clusters[2 * k + 1]]++] = 2 * k;
    }
    if ((rc = upload(e, e->d_nb_off, nb_off))) return bail(rc);
    if ((rc = upload(e, e->d_nb_msg, nb_msg))) return bail(rc);
    if ((rc = upload(e, e->d_sepcl, p.sepset_clusters))) return bail(rc);
    if ((rc = dev_alloc(e, e->d_eps, ns * (size_t)std::max(1, p.n_clusters)))) return bail(rc);
    if ((rc = dev_alloc(e, e->d_thr, 2 * (size_t)(PGBP_MAX_DIM + 1)))) return bail(rc);
    if ((rc = dev_alloc(e, e->d_logtab, 256))) return bail(rc);
    {
      // DevState::logtab, in the host's extended precision
      double tab[256];
      for (int i = 0; i < 128; ++i) {
        const long double c = 0.5L + ((long double)i + 0.5L) / 256.0L;
        const double inv = (double)(1.0L / c);
        tab[2 * i] = inv;
        tab[2 * i + 1] = (double)(-logl((long double)inv));
      }
      if (hipMemcpy(e->d_logtab.get(), tab, sizeof(tab), hipMemcpyHostToDevice) != hipSuccess) return bail(PGBP_ERR_HIP);
    }
  }
  if ((rc = dev_alloc(e, e->d_fail, ns))) return bail(rc);
  if ((rc = dev_alloc(e, e->d_poison, nsw * (size_t)p.n_clusters))) return bail(rc);
  if ((rc = dev_alloc(e, e->d_iscal, ns))) return bail(rc);
  if ((rc = dev_alloc(e, e->d_notcal, ns))) return bail(rc);
  // (the marks of the register-resident kernels are cleared by the kernel that reads them: they start out clear.  On the
  // engine's stream, like every later access.  They are clear between pairs because enqueue_pair_and_iscal has no way out
  // between its traversals and the launch that reads and clears them: enqueue_tree returns nothing and records a failed
  // workspace allocation in enqueue_rc only)
  if (hipMemsetAsync(e->d_notcal.get(), 0, sizeof(int32_t) * ns, e->st) != hipSuccess) return bail(PGBP_ERR_HIP);
  if ((rc = upload(e, e->d_boff, p.boff))) return bail(rc);
  if ((rc = upload(e, e->d_packed_off, p.packed_off))) return bail(rc);
  if ((rc = upload(e, e->d_roff, p.roff))) return bail(rc);
  if ((rc = upload(e, e->d_rpacked_off, p.rpacked_off))) return bail(rc);
  if ((rc = dev_alloc(e, e->d_mu, ns * (size_t)std::max(1, p.max_dim)))) return bail(rc);
  if ((rc = dev_alloc(e, e->d_norm, ns))) return bail(rc);
  if ((rc = dev_alloc(e, e->d_info, ns))) return bail(rc);
  {
    std::vector<int32_t> rdim(nm);
    for (size_t d = 0; d < nm; ++d) rdim[d] = p.dims[p.n_clusters + d / 2];
    for (int32_t v : rdim) e->max_s = std::max(e->max_s, v);
    if ((rc = upload(e, e->d_bdim, p.dims))) return bail(rc);
    if ((rc = upload(e, e->d_rdim, rdim))) return bail(rc);
    if ((rc = dev_alloc(e, e->d_symflag, 1))) return bail(rc);
  }
  if ((rc = dev_alloc(e, e->d_one_task_off, 2))) return bail(rc);
  if ((rc = dev_alloc(e, e->d_one_entry, 1))) return bail(rc);
  if ((rc = dev_alloc(e, e->d_one_rec, 1))) return bail(rc);
  // beliefs = constant function 1 (h, J, g all 0: src/beliefs.jl:108-132); residuals 0;
  // flags false / kldiv -1, empty messages born calibrated (src/beliefs.jl:914-924)
  if (hipMemsetAsync(e->d_pool.get(), 0, ns * p.pool_stride() * sizeof(double), e->st) != hipSuccess ||
      hipMemsetAsync(e->d_fpool.get(), 0, ns * p.cluster_stride() * sizeof(double), e->st) != hipSuccess ||
      hipMemsetAsync(e->d_rpool.get(), 0, ns * p.rpool_stride() * sizeof(double), e->st) != hipSuccess ||
      hipMemsetAsync(e->d_status.get(), 0, nsw * nm * sizeof(int32_t), e->st) != hipSuccess ||
      hipMemsetAsync(e->d_flags.get(), 0, nsw * nm * sizeof(int32_t), e->st) != hipSuccess ||
      hipMemsetAsync(e->d_klflags.get(), 0, nsw * nm * sizeof(int32_t), e->st) != hipSuccess ||
      hipMemsetAsync(e->d_kldiv.get(), 0, nsw * nm * sizeof(double), e->st) != hipSuccess ||
      hipMemsetAsync(e->d_poison.get(), 0, nsw * (size_t)p.n_clusters * sizeof(int32_t), e->st) != hipSuccess ||
      hipMemsetAsync(e->d_fail.get(), 0xFF, ns * sizeof(unsigned long long), e->st) != hipSuccess) {
    e->err = "hipMemsetAsync failed";
    return bail(PGBP_ERR_HIP);
  }
  reset_message_flags(e, 1);
  if (hipStreamSynchronize(e->st) != hipSuccess) {
    e->err = "initialisation kernels failed";
    return bail(PGBP_ERR_HIP);
  }
  *out = up.release();
  return PGBP_OK;
}

int64_t pgbp_packed_size(const pgbp_engine* e) { return e ? e->plan.packed_off.back() : -1; }
int64_t pgbp_residual_size(const pgbp_engine* e) { return e ? e->plan.rpacked_off.back() : -1; }
int32_t pgbp_n_messages(const pgbp_engine* e) { return e ? e->plan.n_msgs() : -1; }
int32_t pgbp_belief_dim(const pgbp_engine* e, int32_t belief) {
  return (e && belief >= 0 && belief < e->plan.n_beliefs()) ? e->plan.dims[belief] : -1;
}

double pgbp_residual_threshold(double divisor, double atol) { return quotient_threshold(divisor, atol); }

int pgbp_sync(pgbp_engine* e) {
  DeviceScope device_scope(e);
  if (!e) return PGBP_ERR_INVALID;
  HIPCHK(e, hipStreamSynchronize(e->st));
  HIPCHK(e, hipGetLastError());  // a launch that failed since the last check (bad grid, LDS size) surfaces here
  return e->take_enqueue_rc();   // ... and so does an enqueue step that was skipped for want of a workspace
}

int pgbp_init_factors_frombeliefs(pgbp_engine* e) {
  DeviceScope device_scope(e);
  if (!e) return PGBP_ERR_INVALID;
  const Plan& p = e->plan;
  if (e->layout_sm)
    HIPCHK(e, hipMemcpyAsync(e->sm.fpool.get(), e->sm.pool.get(), sizeof(double) * (size_t)p.packed_off[p.n_clusters] * (size_t)sm_row(p.n_sites),
                             hipMemcpyDeviceToDevice, e->st));
  else
    launch_copy_strided(e->d_pool.get(), p.pool_stride(), e->d_fpool.get(), p.cluster_stride(), p.cluster_stride(), p.n_sites,
                        e->st);
  e->have_factors = true;
  return pgbp_sync(e);
}

int pgbp_set_beliefs(pgbp_engine* e, const double* packed, int32_t snapshot_factors) {
  DeviceScope device_scope(e);
  if (!e || !packed) return PGBP_ERR_INVALID;
  const Plan& p = e->plan;
  {
    int rc0 = ensure_layout(e, false);  // factors / residuals that stay must be in the layout the upload uses
    if (rc0) return rc0;
    e->sym_known = false;
  }
  const int64_t psz = p.packed_off.back();
  DevBuf<double> stage;
  if (int rc0 = dev_alloc(e, stage, (size_t)psz * p.n_sites)) return rc0;
  hipError_t rc = hipMemcpyAsync(stage.get(), packed, sizeof(double) * (size_t)psz * p.n_sites, hipMemcpyHostToDevice, e->st);
  if (rc == hipSuccess) {
    launch_records(stage.get(), psz, e->d_packed_off.get(), e->d_pool.get(), p.pool_stride(), e->d_boff.get(), e->d_packed_off.get(),
                   p.n_beliefs(), p.n_sites, e->st);
    rc = hipStreamSynchronize(e->st);
  }
  if (rc != hipSuccess) return e->fail(PGBP_ERR_HIP, std::string("pgbp_set_beliefs: ") + hipGetErrorString(rc));
  if (snapshot_factors) return pgbp_init_factors_frombeliefs(e);
  return PGBP_OK;
}

int pgbp_get_beliefs(pgbp_engine* e, double* packed) {
  DeviceScope device_scope(e);
  if (!e || !packed) return PGBP_ERR_INVALID;
  const Plan& p = e->plan;
  {
    int rc0 = ensure_layout(e, false);
    if (rc0) return rc0;
  }
  const int64_t psz = p.packed_off.back();
  DevBuf<double> stage;
  if (int rc0 = dev_alloc(e, stage, (size_t)psz * p.n_sites)) return rc0;
  launch_records(e->d_pool.get(), p.pool_stride(), e->d_boff.get(), stage.get(), psz, e->d_packed_off.get(), e->d_packed_off.get(), p.n_beliefs(),
                 p.n_sites, e->st);
  hipError_t rc = hipMemcpyAsync(packed, stage.get(), sizeof(double) * (size_t)psz * p.n_sites, hipMemcpyDeviceToHost, e->st);
  if (rc == hipSuccess) rc = hipStreamSynchronize(e->st);
  if (rc != hipSuccess) return e->fail(PGBP_ERR_HIP, std::string("pgbp_get_beliefs: ") + hipGetErrorString(rc));
  return PGBP_OK;
}

int pgbp_get_site_beliefs(pgbp_engine* e, int32_t site, double* packed) {
  DeviceScope device_scope(e);
  if (!e || !packed) return PGBP_ERR_INVALID;
  const Plan& p = e->plan;
  if (site < 0 || site >= p.n_sites) return e->fail(PGBP_ERR_INVALID, "site index out of range");
  {
    int rc0 = ensure_layout(e, false);
    if (rc0) return rc0;
  }
  const int64_t psz = p.packed_off.back();
  DevBuf<double> stage;
  if (int rc0 = dev_alloc(e, stage, (size_t)psz)) return rc0;
  launch_records(e->d_pool.get() + (int64_t)site * p.pool_stride(), p.pool_stride(), e->d_boff.get(), stage.get(), psz, e->d_packed_off.get(),
                 e->d_packed_off.get(), p.n_beliefs(), 1, e->st);
  hipError_t rc = hipMemcpyAsync(packed, stage.get(), sizeof(double) * (size_t)psz, hipMemcpyDeviceToHost, e->st);
  if (rc == hipSuccess) rc = hipStreamSynchronize(e->st);
  if (rc != hipSuccess) return e->fail(PGBP_ERR_HIP, std::string("pgbp_get_site_beliefs: ") + hipGetErrorString(rc));
  return PGBP_OK;
}

static int belief_rec(pgbp_engine* e, int32_t site, int32_t b, double** dptr, int64_t* len) {
  const Plan& p = e->plan;
  if (site < 0 || site >= p.n_sites || b < 0 || b >= p.n_beliefs())
    return e->fail(PGBP_ERR_INVALID, "site or belief index out of range");
  *dptr = e->d_pool.get() + (int64_t)site * p.pool_stride() + p.boff[b];
  *len = p.packed_off[b + 1] - p.packed_off[b];
  return PGBP_OK;
}

int pgbp_set_belief(pgbp_engine* e, int32_t site, int32_t belief, const double* rec) {
  DeviceScope device_scope(e);
  if (!e || !rec) return PGBP_ERR_INVALID;
  double* d;
  int64_t len;
  int rc = belief_rec(e, site, belief, &d, &len);
  if (rc) return rc;
  if ((rc = ensure_layout(e, false))) return rc;
  e->sym_known = false;
  HIPCHK(e, hipMemcpyAsync(d, rec, sizeof(double) * len, hipMemcpyHostToDevice, e->st));
  return pgbp_sync(e);
}

int pgbp_get_belief(pgbp_engine* e, int32_t site, int32_t belief, double* rec) {
  DeviceScope device_scope(e);
  if (!e || !rec) return PGBP_ERR_INVALID;
  double* d;
  int64_t len;
  int rc = belief_rec(e, site, belief, &d, &len);
  if (rc) return rc;
  if ((rc = ensure_layout(e, false))) return rc;
  HIPCHK(e, hipMemcpyAsync(rec, d, sizeof(double) * len, hipMemcpyDeviceToHost, e->st));
  return pgbp_sync(e);
}

// The exchange buffer of a cut cluster graph: records gathered on the device into one contiguous buffer (what a
// collective would carry), one copy across the bus.
static int xbuf_prepare(pgbp_engine* e, int32_t site, int32_t n, const int32_t* beliefs, int64_t* total) {
  const Plan& p = e->plan;
  if (site < 0 || site >= p.n_sites || n < 0 || (n > 0 && !beliefs)) return e->fail(PGBP_ERR_INVALID, "site or belief list");
  std::vector<int64_t> off((size_t)2 * n + 1);
  int64_t at = 0;
  for (int32_t i = 0; i < n; ++i) {
    const int32_t b = beliefs[i];
    if (b < 0 || b >= p.n_beliefs()) return e->fail(PGBP_ERR_INVALID, "belief index out of range");
    off[i] = p.boff[b];
    off[(size_t)n + i] = at;
    at += p.packed_off[b + 1] - p.packed_off[b];
  }
  off[(size_t)2 * n] = at;
  *total = at;
  int rc = ensure_layout(e, false);
  if (rc) return rc;
  if ((int64_t)off.size() > e->xoff_cap || at > e->xbuf_cap) HIPCHK(e, hipStreamSynchronize(e->st));
  if ((int64_t)off.size() > e->xoff_cap) {
    e->xoff_cap = 0;
    if ((rc = dev_alloc(e, e->d_xoff, off.size()))) return rc;
    e->xoff_cap = (int64_t)off.size();
  }
  if (at > e->xbuf_cap) {
    e->xbuf_cap = 0;
    if ((rc = dev_alloc(e, e->d_xbuf, (size_t)at))) return rc;
    e->xbuf_cap = std::max<int64_t>(at, 1);
  }
  HIPCHK(e, hipMemcpyAsync(e->d_xoff.get(), off.data(), sizeof(int64_t) * off.size(), hipMemcpyHostToDevice, e->st));
  HIPCHK(e, hipStreamSynchronize(e->st));   // (`off` is a local)
  return PGBP_OK;
}

int64_t pgbp_packed_beliefs_size(pgbp_engine* e, int32_t n, const int32_t* beliefs) {
  if (!e || n < 0 || (n > 0 && !beliefs)) return -1;
  const Plan& p = e->plan;
  int64_t at = 0;
  for (int32_t i = 0; i < n; ++i) {
    if (beliefs[i] < 0 || beliefs[i] >= p.n_beliefs()) return -1;
    at += p.packed_off[beliefs[i] + 1] - p.packed_off[beliefs[i]];
  }
  return at;
}

int pgbp_pack_beliefs(pgbp_engine* e, int32_t site, int32_t n, const int32_t* beliefs, double* buf) {
  DeviceScope device_scope(e);
  if (!e || (n > 0 && !buf)) return PGBP_ERR_INVALID;
  int64_t total = 0;
  int rc = xbuf_prepare(e, site, n, beliefs, &total);
  if (rc || n == 0) return rc;
  launch_pack_records(e->d_pool.get() + (int64_t)site * e->plan.pool_stride(), e->d_xoff.get(), e->d_xoff.get() + n, n, e->d_xbuf.get(), 1, e->st);
  HIPCHK(e, hipGetLastError());
  HIPCHK(e, hipMemcpyAsync(buf, e->d_xbuf.get(), sizeof(double) * (size_t)total, hipMemcpyDeviceToHost, e->st));
  return pgbp_sync(e);
}

int pgbp_unpack_beliefs(pgbp_engine* e, int32_t site, int32_t n, const int32_t* beliefs, const double* buf) {
  DeviceScope device_scope(e);
  if (!e || (n > 0 && !buf)) return PGBP_ERR_INVALID;
  int64_t total = 0;
  int rc = xbuf_prepare(e, site, n, beliefs, &total);
  if (rc || n == 0) return rc;
  e->sym_known = false;
  HIPCHK(e, hipMemcpyAsync(e->d_xbuf.get(), buf, sizeof(double) * (size_t)total, hipMemcpyHostToDevice, e->st));
  launch_pack_records(e->d_pool.get() + (int64_t)site * e->plan.pool_stride(), e->d_xoff.get(), e->d_xoff.get() + n, n, e->d_xbuf.get(), 0, e->st);
  HIPCHK(e, hipGetLastError());
  return pgbp_sync(e);
}

int pgbp_reset_from_factors(pgbp_engine* e) {
  DeviceScope device_scope(e);
  if (!e) return PGBP_ERR_INVALID;
  int rc = reset_from_factors_async(e);
  if (rc) return rc;
  return pgbp_sync(e);
}

int pgbp_reset_flags(pgbp_engine* e, int32_t reset_kl) {
  DeviceScope device_scope(e);
  if (!e) return PGBP_ERR_INVALID;
  reset_message_flags(e, reset_kl);
  return pgbp_sync(e);
}

int pgbp_get_residuals(pgbp_engine* e, double* packed, int32_t* iscalibrated_resid, double* kldiv,
                       int32_t* iscalibrated_kl) {
  DeviceScope device_scope(e);
  if (!e) return PGBP_ERR_INVALID;
  const Plan& p = e->plan;
  if (packed || e->layout_sm) {  // the word arrays are transposed in the site-minor layout
    int rc0 = ensure_layout(e, false);
    if (rc0) return rc0;
  }
  const size_t ns = (size_t)p.n_sites, nm = (size_t)p.n_msgs();
  if (packed) {
    const int64_t rsz = p.rpacked_off.back();
    DevBuf<double> stage;
    if (int rc0 = dev_alloc(e, stage, (size_t)std::max<int64_t>(1, rsz) * ns)) return rc0;
    launch_records(e->d_rpool.get(), p.rpool_stride(), e->d_roff.get(), stage.get(), rsz, e->d_rpacked_off.get(), e->d_rpacked_off.get(),
                   (int)nm, p.n_sites, e->st);
    hipError_t rc = hipMemcpyAsync(packed, stage.get(), sizeof(double) * (size_t)rsz * ns, hipMemcpyDeviceToHost, e->st);
    if (rc == hipSuccess) rc = hipStreamSynchronize(e->st);
    if (rc != hipSuccess) return e->fail(PGBP_ERR_HIP, std::string("pgbp_get_residuals: ") + hipGetErrorString(rc));
  }
  if (iscalibrated_resid)
    HIPCHK(e, hipMemcpyAsync(iscalibrated_resid, e->d_flags.get(), sizeof(int32_t) * ns * nm, hipMemcpyDeviceToHost, e->st));
  if (kldiv) HIPCHK(e, hipMemcpyAsync(kldiv, e->d_kldiv.get(), sizeof(double) * ns * nm, hipMemcpyDeviceToHost, e->st));
  if (iscalibrated_kl)
    HIPCHK(e, hipMemcpyAsync(iscalibrated_kl, e->d_klflags.get(), sizeof(int32_t) * ns * nm, hipMemcpyDeviceToHost, e->st));
  return pgbp_sync(e);
}

int pgbp_get_residual(pgbp_engine* e, int32_t site, int32_t msg, double* rec, int32_t* iscalibrated_resid, double* kldiv,
                      int32_t* iscalibrated_kl) {
  DeviceScope device_scope(e);
  if (!e) return PGBP_ERR_INVALID;
  const Plan& p = e->plan;
  if (site < 0 || site >= p.n_sites || msg < 0 || msg >= p.n_msgs())
    return e->fail(PGBP_ERR_INVALID, "pgbp_get_residual: site or message index out of range");
  int rc = ensure_layout(e, false);   // the record in the ABI's order; the word arrays as [site][message]
  if (rc) return rc;
  const size_t w = (size_t)site * (size_t)p.n_msgs() + (size_t)msg;
  const int64_t len = p.rpacked_off[msg + 1] - p.rpacked_off[msg];
  if (rec && len > 0)
    HIPCHK(e, hipMemcpyAsync(rec, e->d_rpool.get() + (int64_t)site * p.rpool_stride() + p.roff[msg], sizeof(double) * (size_t)len,
                             hipMemcpyDeviceToHost, e->st));
  if (iscalibrated_resid) HIPCHK(e, hipMemcpyAsync(iscalibrated_resid, e->d_flags.get() + w, sizeof(int32_t), hipMemcpyDeviceToHost, e->st));
  if (kldiv) HIPCHK(e, hipMemcpyAsync(kldiv, e->d_kldiv.get() + w, sizeof(double), hipMemcpyDeviceToHost, e->st));
  if (iscalibrated_kl) HIPCHK(e, hipMemcpyAsync(iscalibrated_kl, e->d_klflags.get() + w, sizeof(int32_t), hipMemcpyDeviceToHost, e->st));
  return pgbp_sync(e);
}

int pgbp_set_schedule(pgbp_engine* e, int32_t n_trees, const int32_t* tree_off, const int32_t* pa_j,
                      const int32_t* ch_j) {
  DeviceScope device_scope(e);
  if (!e) return PGBP_ERR_INVALID;
  int rc = plan_set_schedule(e->plan, n_trees, tree_off, pa_j, ch_j);
  if (rc) return e->fail(rc, e->plan.err);  // the previous schedule (if any) stays in force
  HIPCHK(e, hipStreamSynchronize(e->st));
  free_traversals(e);
  e->dpost.resize(n_trees);
  e->dpre.resize(n_trees);
  for (int t = 0; t < n_trees && rc == PGBP_OK; ++t) {
    for (int dir = 0; dir < 2 && rc == PGBP_OK; ++dir) {
      const Traversal& tr = dir == 0 ? e->plan.trees[t].post : e->plan.trees[t].pre;
      DevTraversal d;   // (moved into the engine once every buffer of it exists)
      if ((rc = upload(e, d.d_task_off, tr.task_off))) break;
      if ((rc = upload(e, d.d_entries, tr.entries))) break;
      if (e->plan.max_dim <= 2 && e->plan.n_sites >= 8 && e->max_s <= 1) {
        // thread-per-site kernel for sepsets of at most one variable: every entry as ONE record (URec)
        const Plan& pl = e->plan;
        std::vector<URec> ur(tr.entries.size());
        for (size_t q = 0; q < tr.entries.size(); ++q) {
          const Entry& en = tr.entries[q];
          const MsgDesc& m = pl.msgs[en.msg];
          URec& r = ur[q];
          r = URec{};
          r.msg = en.msg; r.seq = en.seq; r.reuse = en.reuse; r.from_b = m.from_b; r.to_b = m.to_b;
          r.mf = m.mf; r.s = m.s; r.mt = m.mt; r.ni = m.ni;
          r.k = m.s >= 1 ? pl.idxpool[m.keep_map] : 0;
          r.i0 = m.ni >= 1 ? pl.idxpool[m.int_map] : 0;
          r.i1 = m.ni >= 2 ? pl.idxpool[m.int_map + 1] : 0;
          r.u = m.s >= 1 ? pl.idxpool[m.up_map] : 0;
          r.from_off = m.from_off; r.sep_off = m.sep_off; r.to_off = m.to_off; r.res_off = m.res_off;
          r.from_p = pl.packed_off[m.from_b]; r.sep_p = pl.packed_off[m.sep_b]; r.to_p = pl.packed_off[m.to_b];
          r.res_p = pl.rpacked_off[en.msg];
        }
        if ((rc = upload(e, d.d_urecs, ur))) break;
      }
      if ((rc = upload(e, d.d_fentries, tr.fentries))) break;
      if (tr.has_pro) {
        if ((rc = upload(e, d.d_fpros, tr.fpros))) break;
        if ((rc = upload(e, d.d_cpros, tr.cpros))) break;
      }
      if ((rc = upload(e, d.d_centries, tr.centries))) break;
      if ((rc = upload(e, d.d_chunk_wg_off, tr.chunk_wg_off))) break;
      std::vector<int32_t> grp_recs(tr.cgroups);
      for (int32_t& t : grp_recs)
        if (t >= 0) t = tr.task_grec[t];
      if ((rc = upload(e, d.d_cgroups, grp_recs))) break;
      if ((rc = upload(e, d.d_cgroups_task, tr.cgroups))) break;
      if ((rc = upload(e, d.d_grecs, tr.grecs))) break;
      if ((rc = upload(e, d.d_rowmap, tr.rowmap))) break;
      for (size_t q = 0; q < tr.entries.size(); ++q)
        if (e->plan.msgs[tr.entries[q].msg].s > kKlLdsMaxS) d.kl_big.push_back((int32_t)q);
      if ((rc = upload(e, d.d_kl_big, d.kl_big))) break;
      (dir == 0 ? e->dpost[t] : e->dpre[t]) = std::move(d);
    }
    if (rc == PGBP_OK) {
      const Tree& T = e->plan.trees[t];
      e->d_tail.emplace_back();
      e->d_tail_pros.emplace_back();   // (null unless a traversal of this tree has prologues)
      rc = upload(e, e->d_tail.back(), T.tail);
      if (rc == PGBP_OK && (T.post.has_pro || T.pre.has_pro)) rc = upload(e, e->d_tail_pros.back(), T.tail_pros);
    }
  }
  if (rc) {  // out of device memory half way: leave the engine without a schedule rather than with half of one
    free_traversals(e);
    e->plan.trees.clear();
    e->plan.all_fast = false;
  }
  return rc;
}

int pgbp_propagate(pgbp_engine* e, int32_t cluster_to, int32_t sepset, int32_t cluster_from, const pgbp_opts* opts,
                   int32_t* info) {
  DeviceScope device_scope(e);
  if (!e) return PGBP_ERR_INVALID;
  int rc = check_opts(e, opts);
  if (rc) return rc;
  const Plan& p = e->plan;
  const int k = sepset - p.n_clusters;
  if (k < 0 || k >= p.n_sepsets) return e->fail(PGBP_ERR_INVALID, "pgbp_propagate: not a sepset index");
  const int a = p.sepset_clusters[2 * k], b = p.sepset_clusters[2 * k + 1];
  int dir;
  if (cluster_to == a && cluster_from == b)
    dir = 0;
  else if (cluster_to == b && cluster_from == a)
    dir = 1;
  else
    return e->fail(PGBP_ERR_INVALID, "pgbp_propagate: the sepset does not connect these two clusters");
  if ((rc = ensure_layout(e, false))) return rc;  // single messages run on the generic kernel
  const int32_t toff[2] = {0, 1};
  Entry en{2 * k + dir, 0, 0, 0};
  HIPCHK(e, hipMemcpyAsync(e->d_one_task_off.get(), toff, sizeof(toff), hipMemcpyHostToDevice, e->st));
  HIPCHK(e, hipMemcpyAsync(e->d_one_entry.get(), &en, sizeof(en), hipMemcpyHostToDevice, e->st));
  if ((rc = reset_fail(e))) return rc;
  DevState S = dev_state(e, opts);
  if (big_msg(p.msgs[en.msg])) {
    if ((rc = ensure_ws(e, (int64_t)p.n_sites * big_ws_doubles(p.msgs[en.msg].mf)))) return rc;
    launch_level_big(S, e->d_one_task_off.get(), e->d_one_entry.get(), 0, 1, p.n_sites, 0, 0, p.msgs[en.msg].mf, e->d_ws.get(), e->st);
  } else {
    const GRec rec = make_grec(p, en, -1);
    HIPCHK(e, hipMemcpyAsync(e->d_one_rec.get(), &rec, sizeof(rec), hipMemcpyHostToDevice, e->st));
    launch_level_generic(S, e->d_one_rec.get(), 0, 1, p.n_sites, 0, 0, p.msgs[en.msg].mf, false, e->st);
  }
  std::vector<unsigned long long> keys(p.n_sites);
  HIPCHK(e, hipMemcpyAsync(keys.data(), e->d_fail.get(), sizeof(unsigned long long) * p.n_sites, hipMemcpyDeviceToHost, e->st));
  HIPCHK(e, hipStreamSynchronize(e->st));
  HIPCHK(e, hipGetLastError());
  if (info)
    for (int s = 0; s < p.n_sites; ++s)
      info[s] = !is_failure_key(keys[s]) ? 0 : (int32_t)(keys[s] & ((1ull << kInfoBits) - 1));
  return PGBP_OK;
}

int pgbp_residual_kldiv(pgbp_engine* e, int32_t cluster_to, int32_t sepset, int32_t cluster_from, const pgbp_opts* opts,
                        int32_t* iscalibrated_kl) {
  DeviceScope device_scope(e);
  if (!e) return PGBP_ERR_INVALID;
  const Plan& p = e->plan;
  int rc = check_opts(e, opts);
  if (rc) return rc;
  const int k = sepset - p.n_clusters;
  if (k < 0 || k >= p.n_sepsets) return e->fail(PGBP_ERR_INVALID, "pgbp_residual_kldiv: not a sepset index");
  const int a = p.sepset_clusters[2 * k], b = p.sepset_clusters[2 * k + 1];
  int dir;
  if (cluster_to == a && cluster_from == b)
    dir = 0;
  else if (cluster_to == b && cluster_from == a)
    dir = 1;
  else
    return e->fail(PGBP_ERR_INVALID, "pgbp_residual_kldiv: the sepset does not connect these two clusters");
  Entry en{2 * k + dir, 0, 0, 0};
  const int s_msg = p.msgs[en.msg].s;
  const int32_t toff[2] = {0, 1};   // (d_one_task_off[0] = 0 doubles as the list "entry 0" of the workspace instance)
  HIPCHK(e, hipMemcpyAsync(e->d_one_task_off.get(), toff, sizeof(toff), hipMemcpyHostToDevice, e->st));
  HIPCHK(e, hipMemcpyAsync(e->d_one_entry.get(), &en, sizeof(en), hipMemcpyHostToDevice, e->st));
  HIPCHK(e, hipStreamSynchronize(e->st));   // (toff, en: locals)
  const bool kl_ws = s_msg > kKlLdsMaxS;
  if (kl_ws && (rc = ensure_ws(e, (int64_t)p.n_sites * kldiv_ws_doubles(s_msg)))) return rc;
  if (e->layout_sm && (rc = ensure_site_minor(e, false))) return rc;
  DevState S = dev_state(e, opts);
  // a standalone call always computes (stop_below = 0; the status of the last attempt of this message still gates)
  e->kl_flags_clean = e->kl_div_clean = false;
  launch_residual_kldiv(S, e->d_one_entry.get(), 0, 1, s_msg, e->d_kldiv.get(), e->d_klflags.get(), p.n_sites, 0, e->st,
                        kl_ws ? e->d_one_task_off.get() : nullptr, kl_ws ? 1 : 0, e->d_ws.get());
  if (iscalibrated_kl) {
    std::vector<int32_t> all((size_t)p.n_sites * std::max(1, p.n_msgs()));
    HIPCHK(e, hipMemcpyAsync(all.data(), e->d_klflags.get(), sizeof(int32_t) * (size_t)p.n_sites * p.n_msgs(),
                             hipMemcpyDeviceToHost, e->st));
    HIPCHK(e, hipStreamSynchronize(e->st));
    for (int s = 0; s < p.n_sites; ++s) iscalibrated_kl[s] = all[(size_t)s * p.n_msgs() + en.msg];
  }
  HIPCHK(e, hipStreamSynchronize(e->st));
  HIPCHK(e, hipGetLastError());
  return PGBP_OK;
}

int pgbp_regularize_bycluster(pgbp_engine* e) {
  DeviceScope device_scope(e);
  if (!e) return PGBP_ERR_INVALID;
  const Plan& p = e->plan;
  int rc = ensure_layout(e, false);
  if (rc) return rc;
  launch_regularize_bycluster(e->d_pool.get(), p.pool_stride(), e->d_boff.get(), e->d_bdim.get(), e->d_nb_off.get(), e->d_nb_msg.get(), e->d_msgs.get(),
                              e->d_idx.get(), e->d_sepcl.get(), e->d_eps.get(), p.n_clusters, p.n_sepsets, p.n_sites, e->st);
  e->sym_known = false;
  HIPCHK(e, hipGetLastError());
  return PGBP_OK;
}

int pgbp_regularize_onschedule(pgbp_engine* e, int32_t site_begin, int32_t site_end, const pgbp_opts* opts,
                               int32_t* fail_msg, int32_t* fail_info) {
  DeviceScope device_scope(e);
  if (!e) return PGBP_ERR_INVALID;
  const Plan& p = e->plan;
  if (site_begin < 0 || site_end > p.n_sites || site_begin > site_end)
    return e->fail(PGBP_ERR_INVALID, "pgbp_regularize_onschedule: site range outside [0, n_sites]");
  int rc = check_opts(e, opts);
  if (rc) return rc;
  const OnSchedule& os = plan_onschedule(p);
  if (!e->os_ready) {
    OsBufs B;
    if ((rc = upload(e, B.a_cl, os.a_cl)) || (rc = upload(e, B.ed_off, os.ed_off)) || (rc = upload(e, B.ed_msg, os.ed_msg)) ||
        (rc = upload(e, B.task_off, os.task_off)) || (rc = upload(e, B.grecs, os.grecs)) || (rc = upload(e, B.entries, os.entries)))
      return rc;
    e->os = std::move(B);
    e->os_ready = true;
  }
  const int ns = site_end - site_begin;
  if (ns > 0) {
    if ((rc = ensure_layout(e, false))) return rc;   // the plain layout: what pgbp_propagate runs on
    int64_t ws = 0;   // senders above kLdsMaxDim: one workspace slab per (task, site) of their launch
    for (const OnSchedule::Launch& ln : os.launches)
      if (ln.kind == 2) ws = std::max(ws, (int64_t)ln.n * big_ws_doubles(ln.max_mf));
    if (ws > 0 && (rc = ensure_ws(e, ws * ns))) return rc;
    if ((rc = reset_fail(e))) return rc;
    // the range's first site as site 0 of every launch (plain layout: site-major pools and word arrays)
    DevState S = dev_state(e, opts);
    S.pool += (int64_t)site_begin * S.pool_stride;
    S.rpool += (int64_t)site_begin * S.rpool_stride;
    S.flags += (int64_t)site_begin * S.n_msgs;
    S.status += (int64_t)site_begin * S.n_msgs;
    S.fail += site_begin;
    S.poison += (int64_t)site_begin * S.n_clusters;
    // Every level runs on every site, failed or not (stop_below = 0): a failure only stops what is downstream of it
    // (poison), and everything downstream of a message comes later than it in walk order, so the lowest fail key of a
    // site is the walk's first failure.
    for (int L = 0; L < os.n_levels; ++L) {
      launch_regularize_onschedule(S.pool, S.pool_stride, e->d_bdim.get(), e->os.a_cl.get(), os.level_a_off[L],
                                   os.level_a_off[L + 1] - os.level_a_off[L], e->os.ed_off.get(), e->os.ed_msg.get(), e->d_msgs.get(),
                                   e->d_idx.get(), ns, e->st);
      for (int q = os.level_launch_off[L]; q < os.level_launch_off[L + 1]; ++q) {
        const OnSchedule::Launch& ln = os.launches[q];
        if (ln.kind == 0)
          launch_level_generic(S, e->os.grecs.get(), ln.first, ln.n, ns, 0, 0, ln.max_mf, false, e->st);
        else
          launch_level_big(S, e->os.task_off.get(), e->os.entries.get(), ln.first, ln.n, ns, 0, 0, ln.max_mf, e->d_ws.get(), e->st);
      }
    }
    e->sym_known = false;
  }
  std::vector<unsigned long long> keys(std::max(1, ns), kNoFail);
  if (ns > 0)
    HIPCHK(e, hipMemcpyAsync(keys.data(), e->d_fail.get() + site_begin, sizeof(unsigned long long) * ns, hipMemcpyDeviceToHost,
                             e->st));
  HIPCHK(e, hipStreamSynchronize(e->st));
  HIPCHK(e, hipGetLastError());
  for (int s = 0; s < p.n_sites; ++s) {
    const unsigned long long key = s >= site_begin && s < site_end ? keys[s - site_begin] : kNoFail;
    const bool failed = is_failure_key(key);
    if (fail_msg) fail_msg[s] = failed ? os.walk_msg[(size_t)(key >> kInfoBits)] : -1;
    if (fail_info) fail_info[s] = failed ? (int32_t)(key & ((1ull << kInfoBits) - 1)) : 0;
  }
  return PGBP_OK;
}

static int need_schedule(pgbp_engine* e, int tree) {
  if (e->plan.trees.empty()) return e->fail(PGBP_ERR_STATE, "no schedule: call pgbp_set_schedule first");
  if (tree < 0 || tree >= (int)e->plan.trees.size()) return e->fail(PGBP_ERR_INVALID, "schedule tree index out of range");
  return PGBP_OK;
}

static int collect_results(pgbp_engine* e, pgbp_result* results, const std::vector<int32_t>* hist, int n_pairs) {
  const Plan& p = e->plan;
  const int ns = p.n_sites;
  std::vector<unsigned long long> keys(ns);
  std::vector<int32_t> iscal(ns);
  HIPCHK(e, hipMemcpyAsync(keys.data(), e->d_fail.get(), sizeof(unsigned long long) * ns, hipMemcpyDeviceToHost, e->st));
  HIPCHK(e, hipMemcpyAsync(iscal.data(), e->d_iscal.get(), sizeof(int32_t) * ns, hipMemcpyDeviceToHost, e->st));
  HIPCHK(e, hipStreamSynchronize(e->st));
  HIPCHK(e, hipGetLastError());
  if (const int erc = e->take_enqueue_rc()) return erc;
  const int nt = std::max<int>(1, (int)p.trees.size());
  for (int s = 0; s < ns; ++s) {
    pgbp_result r;
    std::memset(&r, 0, sizeof(r));
    r.fail_edge = -1;
    if (is_failure_key(keys[s])) {
      r.succ = 0;
      r.iscal = 0;  // (false, false): src/calibration.jl:82
      decode_fail(e, keys[s], r);
    } else {
      r.succ = 1;
      r.iscal = iscal[s] != 0;
    }
    if (hist && r.succ) {
      for (int q = 0; q < n_pairs; ++q)
        if ((*hist)[(size_t)q * ns + s]) {
          r.iter_reached = q / nt + 1;
          r.tree_reached = q % nt + 1;
          break;
        }
    }
    results[s] = r;
  }
  return PGBP_OK;
}

int pgbp_traverse(pgbp_engine* e, int32_t tree, int32_t dir, const pgbp_opts* opts, pgbp_result* results) {
  DeviceScope device_scope(e);
  if (!e || !results || dir < 0 || dir > 1) return PGBP_ERR_INVALID;
  int rc = check_opts(e, opts);
  if (rc) return rc;
  if ((rc = need_schedule(e, tree))) return rc;
  const Plan& p = e->plan;
  if ((rc = reset_fail(e))) return rc;
  if ((rc = ensure_layout(e, want_bs16(e), want_site_minor(e) && !(opts && opts->update_residualkldiv)))) return rc;
  DevState S = dev_state(e, opts);
  enqueue_tree(e, S, tree, dir == 0 ? 1 : 2, (unsigned long long)tree, opts && opts->update_residualkldiv);
  launch_reduce_flags(e->d_flags.get(), p.n_msgs(), p.n_sites, e->d_iscal.get(), e->st, e->layout_sm ? 1 : 0);
  return collect_results(e, results, nullptr, 0);
}

int pgbp_calibrate(pgbp_engine* e, int32_t niter, const pgbp_opts* opts, pgbp_result* results) {
  DeviceScope device_scope(e);
  if (!e || !results || niter < 0) return PGBP_ERR_INVALID;
  int rc = check_opts(e, opts);
  if (rc) return rc;
  if ((rc = need_schedule(e, 0))) return rc;
  const Plan& p = e->plan;
  const int ns = p.n_sites, nt = (int)p.trees.size();
  if (niter == 0) {  // the loop of src/calibration.jl:46 does not run: (succ, iscal) = (false, false)
    for (int s = 0; s < ns; ++s) {
      std::memset(&results[s], 0, sizeof(pgbp_result));
      results[s].fail_edge = -1;
    }
    return PGBP_OK;
  }
  const bool auto_stop = opts && opts->auto_stop;
  const bool kl = opts && opts->update_residualkldiv;
  const int64_t n_pairs_max = (int64_t)niter * nt;
  if (n_pairs_max > e->hist_cap) {
    e->hist_cap = 0;
    if ((rc = dev_alloc(e, e->d_iscal_hist, (size_t)n_pairs_max * ns))) return rc;
    e->hist_cap = n_pairs_max;
  }
  if ((rc = reset_fail(e))) return rc;
  HIPCHK(e, hipMemsetAsync(e->d_iscal.get(), 0, sizeof(int32_t) * ns, e->st));
  if ((rc = ensure_layout(e, want_bs16(e), want_site_minor(e) && !(opts && opts->update_residualkldiv)))) return rc;
  DevState S = dev_state(e, opts);
  int pairs_done = 0;
  bool stop = false;
  std::vector<int32_t> now;
  std::vector<unsigned long long> keys(ns);
  // `auto`: kAhead schedule trees are enqueued per host round trip.  The device halts EACH SITE at the first tree at which
  // that site is calibrated (a key without failure information is min-ed into the site's fail word right behind that
  // tree's flag reduction, so every traversal enqueued after it returns at its first instruction for that site) and the
  // host reads back which tree that was: every site's beliefs are those of src/calibration.jl:53-56 run on that site
  // alone, at a fraction of the round trips.  The loop ends when every site has reached calibration or failed.
  constexpr int kAhead = 4;
  const unsigned long long stride = seq_stride(e);
  int batch_first = 0;
  std::vector<char> site_done(ns, 0);
  int n_done = 0, last_needed = 0;   // last_needed: one past the last tree at which some site was still running
  for (int i = 0; i < niter && !stop; ++i) {
    for (int j = 0; j < nt && !stop; ++j) {
      const unsigned long long pair = (unsigned long long)i * nt + j;
      enqueue_pair_and_iscal(e, S, j, pair, kl, e->d_iscal_hist.get() + pair * ns);
      ++pairs_done;
      if (!auto_stop) continue;
      launch_halt_if_calibrated(e->d_iscal_hist.get() + pair * ns, e->d_fail.get(), ((pair + 1) * stride - 1) << kInfoBits, ns, e->st);
      const bool last = (i == niter - 1 && j == nt - 1);
      if (pairs_done - batch_first < kAhead && !last) continue;
      const int nb = pairs_done - batch_first;
      now.resize((size_t)nb * ns);
      HIPCHK(e, hipMemcpyAsync(now.data(), e->d_iscal_hist.get() + (size_t)batch_first * ns, sizeof(int32_t) * now.size(), hipMemcpyDeviceToHost, e->st));
      HIPCHK(e, hipMemcpyAsync(keys.data(), e->d_fail.get(), sizeof(unsigned long long) * ns, hipMemcpyDeviceToHost, e->st));
      HIPCHK(e, hipStreamSynchronize(e->st));
      for (int s = 0; s < ns; ++s) {
        if (site_done[s]) continue;
        int reached = -1;
        for (int q = 0; q < nb && reached < 0; ++q)
          if (now[(size_t)q * ns + s] != 0) reached = batch_first + q;
        if (reached >= 0 || is_failure_key(keys[s])) {
          site_done[s] = 1;
          ++n_done;
          // (a failed site: its traversals stopped on their own somewhere in this batch)
          last_needed = std::max(last_needed, reached >= 0 ? reached + 1 : pairs_done);
        }
      }
      if (n_done == ns) {
        pairs_done = last_needed;   // the trees enqueued behind it did nothing, for any site
        stop = true;
      }
      batch_first = pairs_done;
    }
  }
  std::vector<int32_t> hist((size_t)std::max(1, pairs_done) * ns, 0);
  if (pairs_done > 0) {
    HIPCHK(e, hipMemcpyAsync(hist.data(), e->d_iscal_hist.get(), sizeof(int32_t) * (size_t)pairs_done * ns, hipMemcpyDeviceToHost, e->st));
    HIPCHK(e, hipMemcpyAsync(e->d_iscal.get(), e->d_iscal_hist.get() + (size_t)(pairs_done - 1) * ns, sizeof(int32_t) * ns, hipMemcpyDeviceToDevice, e->st));
  }
  return collect_results(e, results, &hist, pairs_done);
}

int pgbp_integrate(pgbp_engine* e, int32_t belief, double* mu, double* norm, int32_t* info) {
  DeviceScope device_scope(e);
  if (!e || !norm) return PGBP_ERR_INVALID;
  const Plan& p = e->plan;
  if (belief < 0 || belief >= p.n_beliefs()) return e->fail(PGBP_ERR_INVALID, "belief index out of range");
  const int m = p.dims[belief];
  const int ns = p.n_sites;
  integrate_async(e, belief, mu ? e->d_mu.get() : nullptr);
  HIPCHK(e, hipMemcpyAsync(norm, e->d_norm.get(), sizeof(double) * ns, hipMemcpyDeviceToHost, e->st));
  std::vector<double> mus;
  if (mu && m > 0) {
    mus.resize((size_t)ns * std::max(1, p.max_dim));
    HIPCHK(e, hipMemcpyAsync(mus.data(), e->d_mu.get(), sizeof(double) * mus.size(), hipMemcpyDeviceToHost, e->st));
  }
  std::vector<int32_t> inf(ns);
  HIPCHK(e, hipMemcpyAsync(inf.data(), e->d_info.get(), sizeof(int32_t) * ns, hipMemcpyDeviceToHost, e->st));
  HIPCHK(e, hipStreamSynchronize(e->st));
  HIPCHK(e, hipGetLastError());
  if (const int erc = e->take_enqueue_rc()) return erc;
  if (mu && m > 0)
    for (int s = 0; s < ns; ++s)
      std::memcpy(mu + (size_t)s * m, mus.data() + (size_t)s * std::max(1, p.max_dim), sizeof(double) * m);
  if (info) std::copy(inf.begin(), inf.end(), info);
  return PGBP_OK;
}

// ---- scores ---------------------------------------------------------------------------------------------

int pgbp_free_energy(pgbp_engine* e, double* out3, int32_t* info) {
  DeviceScope device_scope(e);
  if (!e || !out3) return PGBP_ERR_INVALID;
  if (!e->have_factors) return e->fail(PGBP_ERR_STATE, "pgbp_free_energy: no factors (pgbp_set_beliefs with snapshot, or pgbp_init_factors_frombeliefs)");
  if (e->layout_sm) {
    const int rc0 = ensure_site_minor(e, false);
    if (rc0) return rc0;
  }
  const Plan& p = e->plan;
  const int ns = p.n_sites;
  // beliefs whose [J | J_t | h] does not fit a CU's LDS whole (more than kFreeEnergyLdsMaxDim variables): a second
  // launch, their working matrix in the workspace
  std::vector<int32_t> big;
  for (int b = 0; b < p.n_beliefs(); ++b)
    if (p.dims[b] > kFreeEnergyLdsMaxDim) big.push_back(b);
  DevBuf<double> d_contrib, d_out;
  DevBuf<int32_t> d_inf, d_big;
  int rc;
  if (!big.empty()) {
    if ((rc = ensure_ws(e, (int64_t)big.size() * ns * free_energy_ws_doubles(p.max_dim)))) return rc;
    if ((rc = upload(e, d_big, big))) return rc;
  }
  if ((rc = dev_alloc(e, d_contrib, (size_t)2 * ns * p.n_beliefs()))) return rc;
  if ((rc = dev_alloc(e, d_out, (size_t)3 * ns))) return rc;
  if ((rc = dev_alloc(e, d_inf, (size_t)ns))) return rc;
  std::vector<int32_t> inf(ns, 0x7fffffff);
  hipError_t herr = hipMemcpyAsync(d_inf.get(), inf.data(), sizeof(int32_t) * ns, hipMemcpyHostToDevice, e->st);
  if (herr == hipSuccess) {
    launch_free_energy(e->d_pool.get(), p.pool_stride(), e->d_fpool.get(), p.cluster_stride(), e->d_boff.get(), e->d_bdim.get(), p.n_clusters,
                       p.n_beliefs(), p.max_dim, e->layout_bs16 ? 1 : 0, p.fast_p, d_contrib.get(), d_out.get(), d_inf.get(), ns, e->st,
                       d_big.get(), (int)big.size(), e->d_ws.get());
    herr = hipMemcpyAsync(out3, d_out.get(), sizeof(double) * 3 * ns, hipMemcpyDeviceToHost, e->st);
  }
  if (herr == hipSuccess) herr = hipMemcpyAsync(inf.data(), d_inf.get(), sizeof(int32_t) * ns, hipMemcpyDeviceToHost, e->st);
  if (herr == hipSuccess) herr = hipStreamSynchronize(e->st);
  if (herr == hipSuccess) herr = hipGetLastError();
  if (herr != hipSuccess) return e->fail(PGBP_ERR_HIP, std::string("pgbp_free_energy: ") + hipGetErrorString(herr));
  if (info)
    for (int s = 0; s < ns; ++s) info[s] = inf[s] == 0x7fffffff ? 0 : inf[s];
  return PGBP_OK;
}

// ---- device factor assignment (homogeneous BM on a tree) ----------------------------------------

int pgbp_bm_tree_setup(pgbp_engine* e, const pgbp_bm_tree* t) {
  DeviceScope device_scope(e);
  if (!e || !t || !t->kind || !t->length || !t->data_row || t->p <= 0 || t->p > PGBP_MAX_DIM || t->n_rows < 0)
    return PGBP_ERR_INVALID;
  const Plan& p = e->plan;
  const int nc = p.n_clusters;
  // the cluster dimensions must be what the factor kinds imply
  for (int c = 0; c < nc; ++c) {
    const int k = t->kind[c];
    const int want = k == 0 ? 2 * t->p : (k == 1 || k == 2) ? t->p : (k == 3 ? 0 : p.dims[c]);
    if (k < -1 || k > 3 || p.dims[c] != want || (k >= 0 && !(t->length[c] > 0.0)) ||
        (k >= 2 && (t->data_row[c] < 0 || t->data_row[c] >= t->n_rows)))
      return e->fail(PGBP_ERR_INVALID, "pgbp_bm_tree_setup: cluster " + std::to_string(c) + ": kind, dimension, branch length or data row inconsistent");
  }
  if (t->n_rows > 0 && !t->data) return e->fail(PGBP_ERR_INVALID, "pgbp_bm_tree_setup: data missing");
  BmBufs B;   // (a failure leaves the previous set-up in force)
  int rc;
  if ((rc = upload(e, B.kind, std::vector<int32_t>(t->kind, t->kind + nc)))) return rc;
  if ((rc = upload(e, B.row, std::vector<int32_t>(t->data_row, t->data_row + nc)))) return rc;
  if ((rc = upload(e, B.length, std::vector<double>(t->length, t->length + nc)))) return rc;
  if ((rc = dev_alloc(e, B.ithl, (size_t)nc))) return rc;
  launch_bm_ithl(B.length.get(), B.kind.get(), t->p, B.ithl.get(), nc, e->st);
  const size_t nd = (size_t)p.n_sites * t->n_rows * t->p;
  if ((rc = dev_alloc(e, B.data, nd))) return rc;
  if (nd) HIPCHK(e, hipMemcpy(B.data.get(), t->data, nd * sizeof(double), hipMemcpyHostToDevice));
  if (t->p == 1 && t->n_rows > 0) {   // univariate batches: [row][site] copy for the thread-per-site fill
    if ((rc = dev_alloc(e, B.data_sm, (size_t)t->n_rows * (size_t)sm_row(p.n_sites)))) return rc;
    launch_transpose_words_f64(B.data.get(), B.data_sm.get(), t->n_rows, p.n_sites, 1, e->st);
    HIPCHK(e, hipStreamSynchronize(e->st));
  }
  if ((rc = dev_alloc(e, B.Rinv, (size_t)p.n_sites * t->p * t->p))) return rc;
  if ((rc = dev_alloc(e, B.logdet, (size_t)p.n_sites))) return rc;
  if ((rc = dev_alloc(e, B.mu, (size_t)p.n_sites * t->p))) return rc;
  e->bm = std::move(B);
  e->bm_p = t->p;
  e->bm_rows = t->n_rows;
  e->bm_ready = true;
  return PGBP_OK;
}

// also_factors: assignfactors! followed by init_factors_frombeliefs! (what the callers of the optimisers do once);
// without it only the beliefs are written, as in the body of score() (src/calibration.jl:205-209).
static int bm_fill_async(pgbp_engine* e, bool also_factors, bool skip_sepsets = false) {
  const Plan& p = e->plan;
  if (e->layout_sm && e->bm_p == 1) {  // univariate batch, site-minor state
    launch_bm_tree_fill_uni_sm(e->sm.pool.get(), also_factors ? e->sm.fpool.get() : nullptr, e->d_packed_off.get(), e->d_bdim.get(),
                               e->bm.kind.get(), e->bm.length.get(), e->bm.row.get(), e->bm.data_sm.get(), e->bm_rows, e->bm.Rinv.get(),
                               e->bm.logdet.get(), e->bm.mu.get(), e->bm_per_site, p.n_clusters, p.n_sites, e->st);
    const int64_t nc = p.packed_off[p.n_clusters] * sm_row(p.n_sites), nall = p.packed_off.back() * sm_row(p.n_sites);
    if (!skip_sepsets) HIPCHK(e, hipMemsetAsync(e->sm.pool.get() + nc, 0, sizeof(double) * (size_t)(nall - nc), e->st));  // sepsets = 1
    reset_message_flags(e, also_factors ? 1 : 0);
    if (also_factors) e->have_factors = true;
    return PGBP_OK;
  }
  if (e->layout_sm) {
    const int rc0 = ensure_site_minor(e, false);
    if (rc0) return rc0;
  }
  double* fp = also_factors ? e->d_fpool.get() : nullptr;
  bool done = false;
  if (e->bm_p == p.fast_p)  // lane-blocked instance: every cluster has dimension 0, p or 2p (checked at setup)
    done = launch_bm_tree_fill_fast(e->d_pool.get(), p.pool_stride(), fp, p.cluster_stride(), e->d_boff.get(), e->d_bdim.get(), e->bm.kind.get(),
                                    e->bm.ithl.get(), e->bm.row.get(), e->bm.data.get(), e->bm_rows, e->bm_p, e->bm.Rinv.get(),
                                    e->bm.logdet.get(), e->bm.mu.get(), e->bm_per_site, e->layout_bs16 ? 1 : 0, p.n_clusters,
                                    p.n_sites, e->st);
  if (!done) {
    launch_bm_tree_fill(e->d_pool.get(), p.pool_stride(), e->d_fpool.get(), p.cluster_stride(), e->d_boff.get(), e->d_bdim.get(), e->bm.kind.get(),
                        e->bm.length.get(), e->bm.row.get(), e->bm.data.get(), e->bm_rows, e->bm_p, e->bm.Rinv.get(), e->bm.logdet.get(),
                        e->bm.mu.get(), e->bm_per_site, e->layout_bs16 ? 1 : 0, p.fast_p, p.n_clusters, p.n_sites, e->st);
    also_factors = true;  // the general kernel always writes both
  }
  if (!skip_sepsets)
    launch_zero_strided(e->d_pool.get() + p.cluster_stride(), p.pool_stride(), p.pool_stride() - p.cluster_stride(),
                        p.n_sites, e->st);  // sepsets = 1 (init_beliefs_reset!)
  reset_message_flags(e, also_factors ? 1 : 0);
  if (also_factors) e->have_factors = true;
  return PGBP_OK;
}

int pgbp_bm_tree_assignfactors(pgbp_engine* e, const double* Rinv, const double* logdetR, const double* mu,
                               int32_t per_site) {
  DeviceScope device_scope(e);
  if (!e || !Rinv || !logdetR || !mu) return PGBP_ERR_INVALID;
  if (!e->bm_ready) return e->fail(PGBP_ERR_STATE, "pgbp_bm_tree_assignfactors: call pgbp_bm_tree_setup first");
  const size_t n = per_site ? (size_t)e->plan.n_sites : 1, pp = (size_t)e->bm_p;
  HIPCHK(e, hipMemcpyAsync(e->bm.Rinv.get(), Rinv, n * pp * pp * sizeof(double), hipMemcpyHostToDevice, e->st));
  HIPCHK(e, hipMemcpyAsync(e->bm.logdet.get(), logdetR, n * sizeof(double), hipMemcpyHostToDevice, e->st));
  HIPCHK(e, hipMemcpyAsync(e->bm.mu.get(), mu, n * pp * sizeof(double), hipMemcpyHostToDevice, e->st));
  e->bm_per_site = per_site ? 1 : 0;
  // R^-1 is symmetric and the fill writes symmetric blocks: the layout the traversals want can be kept
  e->sym_known = true;
  e->sym_ok = true;
  if (want_site_minor(e) && e->bm_p == 1 && !e->layout_sm) {  // univariate batch: fill straight in the site-minor layout
    const int rc = ensure_layout(e, false, true);
    if (rc) return rc;
  }
  return bm_fill_async(e, true);
}

int pgbp_enqueue_loglik_bm(pgbp_engine* e, int32_t reps, const pgbp_opts* opts) {
  DeviceScope device_scope(e);
  if (!e) return PGBP_ERR_INVALID;
  int rc = check_opts(e, opts);
  if (rc) return rc;
  if ((rc = need_schedule(e, 0))) return rc;
  if (!e->bm_ready) return e->fail(PGBP_ERR_STATE, "pgbp_enqueue_loglik_bm: call pgbp_bm_tree_setup / assignfactors first");
  if ((rc = reset_fail(e))) return rc;
  if ((rc = ensure_layout(e, want_bs16(e), want_site_minor(e)))) return rc;
  DevState S = dev_state(e, opts);
  const Plan& p = e->plan;
  for (int r = 0; r < reps; ++r) {
    DevState S1 = S;
    S1.sep_zero = fresh_sepsets_shortcut(e) ? 1 : 0;
    if ((rc = bm_fill_async(e, false, S1.sep_zero != 0))) return rc;   // assignfactors!        calibration.jl:205-209
    enqueue_tree(e, S1, 0, 1, 0);                                // postorder             :210
    const int root = p.trees[0].pa.empty() ? 0 : p.trees[0].pa[0];
    integrate_async(e, root, nullptr);  // :212
  }
  return e->take_enqueue_rc();
}

// ---- device factor assignment (any linear-Gaussian model, trees and networks) ---------------------------

int pgbp_lg_setup(pgbp_engine* e, const pgbp_lg_families* f) {
  DeviceScope device_scope(e);
  if (!e) return PGBP_ERR_INVALID;
  const Plan& p = e->plan;
  // a whole model into a local: the engine takes it once the last buffer exists, and until then keeps the one it had.  A new
  // table so carries no parameters, shifts, tip noise or topology
  auto L = std::make_unique<LgModel>();
  std::string why;
  if (!lg_table_build(f, p.dims.data(), p.n_clusters, p.n_sites, p.max_dim, L->T, why))
    return why.empty() ? PGBP_ERR_INVALID : e->fail(PGBP_ERR_INVALID, why);
  const LgTable& T = L->T;
  const int pp = T.p;
  int rc;
  LgBufs& B = L->bufs;
  if ((rc = upload(e, B.off, T.cl_off))) return rc;
  if ((rc = upload(e, B.fam, T.cl_fam))) return rc;
  if ((rc = upload(e, B.np, T.n_parents))) return rc;
  if ((rc = upload(e, B.cp, T.child_pos))) return rc;
  if ((rc = upload(e, B.row, T.data_row))) return rc;
  if ((rc = upload(e, B.pp, T.parent_pos))) return rc;
  if ((rc = upload(e, B.col, T.color))) return rc;
  if ((rc = upload(e, B.len, T.length))) return rc;
  if ((rc = upload(e, B.gam, T.gamma))) return rc;
  const size_t nd = (size_t)p.n_sites * T.n_rows * pp;
  if ((rc = dev_alloc(e, B.data, nd))) return rc;
  if (f->child_mask && (rc = upload(e, B.cm, T.child_mask))) return rc;
  if (f->parent_mask && (rc = upload(e, B.pm, T.parent_mask))) return rc;
  if (nd) {
    if (!f->child_mask) {  // complete data: checked finite
      HIPCHK(e, hipMemcpy(B.data.get(), f->data, nd * sizeof(double), hipMemcpyHostToDevice));
    } else {               // masked-out entries may be NaN on the host: never let them reach arithmetic
      std::vector<double> clean(f->data, f->data + nd);
      for (double& x : clean) if (!std::isfinite(x)) x = 0.0;
      HIPCHK(e, hipMemcpy(B.data.get(), clean.data(), nd * sizeof(double), hipMemcpyHostToDevice));
    }
  }
  const size_t ns = (size_t)p.n_sites;
  if ((rc = dev_alloc(e, B.R, ns * T.n_rates * pp * pp))) return rc;
  if ((rc = dev_alloc(e, B.alpha, ns))) return rc;
  if ((rc = dev_alloc(e, B.theta, ns * pp))) return rc;
  if ((rc = dev_alloc(e, B.mu, ns * pp))) return rc;
  if (T.uni_ok && T.n_rows > 0) {   // the thread-per-site fill reads the tip data with lanes = sites: keep a [row][site] copy
    if ((rc = dev_alloc(e, B.data_sm, (size_t)T.n_rows * (size_t)sm_row(p.n_sites)))) return rc;
    launch_transpose_words_f64(B.data.get(), B.data_sm.get(), T.n_rows, p.n_sites, 1, e->st);
    HIPCHK(e, hipStreamSynchronize(e->st));
  }
  if (!T.simple.empty() && (rc = upload(e, B.simple, T.simple))) return rc;
  L->F = LgStatic{pp, T.K, T.n_rates, T.n_rows, B.off.get(), B.fam.get(), B.np.get(), B.cp.get(), B.row.get(), B.pp.get(), B.len.get(),
                  B.gam.get(), B.col.get(), B.data.get(), B.cm.get(), B.pm.get(), B.data_sm.get(), B.simple.get()};
  e->lg = std::move(L);
  return PGBP_OK;
}

// also_factors: assignfactors! followed by init_factors_frombeliefs!; without it only the beliefs are written, as in
// the body of score() (src/calibration.jl:205-209)
static int lg_fill_async(pgbp_engine* e, bool also_factors, bool skip_sepsets = false) {
  const Plan& p = e->plan;
  const LgModel& L = *e->lg;
  // the displacement correction: the shifted clusters, or with painted optima in force their union with the painted ones
  const LgOptima Op = L.optima_in_force();
  const LgCladeShifts Cs = L.clade_in_force();   // per-site clade shifts of the optimum: a correction of their own, after the noise's
  const int32_t* dcl = Op.regime ? L.disp_cl.get() : L.shift_bufs.cl.get();
  const int32_t n_dcl = Op.regime ? L.n_disp_cl : L.n_shift_cl;
  if (e->layout_sm && L.T.uni_ok) {
    launch_lg_fill_uni_sm(L.F, L.M, e->sm.pool.get(), also_factors ? e->sm.fpool.get() : nullptr, e->d_packed_off.get(), e->d_bdim.get(),
                          p.n_clusters, p.n_sites, e->st);
    launch_lg_shift_uni_sm(L.F, L.M, L.Sh, Op, dcl, n_dcl, e->sm.pool.get(),
                           also_factors ? e->sm.fpool.get() : nullptr, e->d_packed_off.get(), e->d_bdim.get(), p.n_sites, e->st);
    launch_lg_noise_uni_sm(L.F, L.M, L.Sh, Op, L.Nz, L.noise_bufs.cl.get(), L.n_noise_cl, e->sm.pool.get(),
                           also_factors ? e->sm.fpool.get() : nullptr, e->d_packed_off.get(), e->d_bdim.get(), p.n_sites, e->st);
    launch_lg_clade_shift(L.F, L.M, L.Sh, Op, L.Nz, Cs, L.clade_bufs.cl.get(), L.n_clade_cl, 1, e->sm.pool.get(), sm_row(p.n_sites),
                          also_factors ? e->sm.fpool.get() : nullptr, sm_row(p.n_sites), e->d_packed_off.get(), e->d_bdim.get(),
                          p.n_sites, e->st);
    launch_lg_sitemiss(L.F, L.M, L.Sh, Op, L.Nz, L.Ms, Cs, L.miss_bufs.cl.get(), (int)L.miss.cl.size(), 1, e->sm.pool.get(), sm_row(p.n_sites),
                       also_factors ? e->sm.fpool.get() : nullptr, sm_row(p.n_sites), e->d_packed_off.get(), e->d_bdim.get(), p.n_sites,
                       e->st);
    const int64_t nc = p.packed_off[p.n_clusters] * sm_row(p.n_sites), nall = p.packed_off.back() * sm_row(p.n_sites);
    if (!skip_sepsets) HIPCHK(e, hipMemsetAsync(e->sm.pool.get() + nc, 0, sizeof(double) * (size_t)(nall - nc), e->st));  // sepsets = 1
  } else {
    if (e->layout_sm) {
      const int rc0 = ensure_site_minor(e, false);
      if (rc0) return rc0;
    }
    launch_lg_fill(L.F, L.M, e->d_pool.get(), p.pool_stride(), also_factors ? e->d_fpool.get() : nullptr, p.cluster_stride(),
                   e->d_boff.get(), e->d_bdim.get(), e->layout_bs16 ? 1 : 0, p.fast_p, p.max_dim, p.n_clusters, p.n_sites, e->st);
    launch_lg_shift(L.F, L.M, L.Sh, Op, dcl, n_dcl, e->d_pool.get(), p.pool_stride(),
                    also_factors ? e->d_fpool.get() : nullptr, p.cluster_stride(), e->d_boff.get(), e->d_bdim.get(),
                    e->layout_bs16 ? 1 : 0, p.fast_p, p.max_dim, p.n_sites, e->st);
    launch_lg_noise(L.F, L.M, L.Sh, Op, L.Nz, L.noise_bufs.cl.get(), L.n_noise_cl, e->d_pool.get(), p.pool_stride(),
                    also_factors ? e->d_fpool.get() : nullptr, p.cluster_stride(), e->d_boff.get(), e->d_bdim.get(),
                    e->layout_bs16 ? 1 : 0, p.fast_p, L.noise_max_dim, p.n_sites, e->st);
    if (L.Ms.words && e->layout_bs16)   // (a thread-per-site engine is never in the packed layout)
      return e->fail(PGBP_ERR_STATE, "a per-site mask of missing tips is in force but the engine is in the packed layout");
    if (Cs.family && e->layout_bs16)
      return e->fail(PGBP_ERR_STATE, "per-site clade shifts of the optimum are in force but the engine is in the packed layout");
    launch_lg_clade_shift(L.F, L.M, L.Sh, Op, L.Nz, Cs, L.clade_bufs.cl.get(), L.n_clade_cl, 0, e->d_pool.get(), p.pool_stride(),
                          also_factors ? e->d_fpool.get() : nullptr, p.cluster_stride(), e->d_boff.get(), e->d_bdim.get(), p.n_sites,
                          e->st);
    launch_lg_sitemiss(L.F, L.M, L.Sh, Op, L.Nz, L.Ms, Cs, L.miss_bufs.cl.get(), (int)L.miss.cl.size(), 0, e->d_pool.get(), p.pool_stride(),
                       also_factors ? e->d_fpool.get() : nullptr, p.cluster_stride(), e->d_boff.get(), e->d_bdim.get(), p.n_sites,
                       e->st);
    if (!skip_sepsets)
      launch_zero_strided(e->d_pool.get() + p.cluster_stride(), p.pool_stride(), p.pool_stride() - p.cluster_stride(),
                          p.n_sites, e->st);  // sepsets = 1 (init_beliefs_reset!)
  }
  reset_message_flags(e, also_factors ? 1 : 0);
  if (also_factors) e->have_factors = true;
  return PGBP_OK;
}

int pgbp_lg_assignfactors(pgbp_engine* e, const pgbp_lg_params* m) {
  DeviceScope device_scope(e);
  if (!e || !m || !m->R || !m->mu) return PGBP_ERR_INVALID;
  if (!e->lg) return e->fail(PGBP_ERR_STATE, "pgbp_lg_assignfactors: call pgbp_lg_setup first");
  if (m->model != PGBP_LG_BM && m->model != PGBP_LG_OU) return e->fail(PGBP_ERR_INVALID, "pgbp_lg_assignfactors: unknown model");
  if (m->model == PGBP_LG_OU && (!m->alpha || !m->theta))
    return e->fail(PGBP_ERR_INVALID, "pgbp_lg_assignfactors: the OU model needs alpha and theta");
  LgModel& L = *e->lg;
  const LgBufs& B = L.bufs;
  const size_t n = m->per_site ? (size_t)e->plan.n_sites : 1, pp = (size_t)L.T.p;
  HIPCHK(e, hipMemcpyAsync(B.R.get(), m->R, n * L.T.n_rates * pp * pp * sizeof(double), hipMemcpyHostToDevice, e->st));
  HIPCHK(e, hipMemcpyAsync(B.mu.get(), m->mu, n * pp * sizeof(double), hipMemcpyHostToDevice, e->st));
  if (m->alpha) HIPCHK(e, hipMemcpyAsync(B.alpha.get(), m->alpha, n * sizeof(double), hipMemcpyHostToDevice, e->st));
  if (m->theta) HIPCHK(e, hipMemcpyAsync(B.theta.get(), m->theta, n * pp * sizeof(double), hipMemcpyHostToDevice, e->st));
  HIPCHK(e, hipStreamSynchronize(e->st));  // the host buffers may go away
  L.M = LgParams{m->model, m->per_site ? 1 : 0, B.R.get(), B.alpha.get(), m->theta ? B.theta.get() : nullptr, B.mu.get()};
  L.have_params = true;
  // the fill writes exactly symmetric blocks: the layout the traversals want can be kept
  e->sym_known = true;
  e->sym_ok = true;
  // a univariate batch is filled straight in the site-minor layout its traversals use (the wavefront-per-cluster
  // kernel would spend one workgroup per (cluster, site))
  if (want_site_minor(e) && L.T.uni_ok && !e->layout_sm) {
    const int rc = ensure_layout(e, false, true);
    if (rc) return rc;
  }
  return lg_fill_async(e, true);
}

// The setters: every check (the table's: pgbp_lgtable.hpp) before anything changes; new buffers into a local group that
// the model takes once every copy has been made.

// the sorted union of two sorted cluster lists on the device (one word at least), uploaded synchronously: what the displacement
// correction visits when shifts and painted optima are both in force
static int lg_union_clusters(pgbp_engine* e, const std::vector<int32_t>& a, const std::vector<int32_t>& b, DevBuf<int32_t>& out,
                             int32_t* n = nullptr) {
  std::vector<int32_t> u;
  std::set_union(a.begin(), a.end(), b.begin(), b.end(), std::back_inserter(u));
  if (n) *n = (int32_t)u.size();
  if (u.empty()) u.push_back(0);
  return upload(e, out, u);
}

int pgbp_lg_set_edges(pgbp_engine* e, const double* length, const double* gamma) {
  DeviceScope device_scope(e);
  if (!e) return PGBP_ERR_INVALID;
  if (!e->lg) return e->fail(PGBP_ERR_STATE, "pgbp_lg_set_edges: no family table (call pgbp_lg_setup first)");
  LgModel& L = *e->lg;
  std::string why;
  if (!L.T.check_edges(length, gamma, why)) return e->fail(PGBP_ERR_INVALID, why);
  const size_t bytes = (size_t)L.T.n_families * L.T.K * sizeof(double);
  if (length && bytes) HIPCHK(e, hipMemcpyAsync(L.bufs.len.get(), length, bytes, hipMemcpyHostToDevice, e->st));
  if (gamma && bytes) HIPCHK(e, hipMemcpyAsync(L.bufs.gam.get(), gamma, bytes, hipMemcpyHostToDevice, e->st));
  L.T.set_edges(length, gamma);
  if (!L.T.simple.empty())   // the per-cluster records of the thread-per-site fill carry their own copies
    HIPCHK(e, hipMemcpyAsync(L.bufs.simple.get(), L.T.simple.data(), L.T.simple.size() * sizeof(LgSimpleFam),
                             hipMemcpyHostToDevice, e->st));
  HIPCHK(e, hipStreamSynchronize(e->st));  // the host buffers may go away
  return PGBP_OK;
}

int pgbp_lg_set_shifts(pgbp_engine* e, int32_t n_shifts, const int32_t* edge, const double* value, int32_t per_site) {
  DeviceScope device_scope(e);
  if (!e) return PGBP_ERR_INVALID;
  if (!e->lg) return e->fail(PGBP_ERR_STATE, "pgbp_lg_set_shifts: no family table (call pgbp_lg_setup first)");
  LgModel& L = *e->lg;
  std::vector<int32_t> slot, cl;   // the slot table, and the clusters that hold a shifted family, in index order
  std::string why;
  if (!L.T.shift_list(n_shifts, edge, value, per_site, slot, cl, why)) return e->fail(PGBP_ERR_INVALID, why);
  const int pp = L.T.p;
  const size_t ns = per_site ? (size_t)e->plan.n_sites : 1, n = (size_t)n_shifts;
  DevBuf<int32_t> ucl;   // with painted optima in force: the clusters of either list, for the displacement correction
  int rc0;
  if (n_shifts == 0) {   // clear (kernels already enqueued may still read the old shifts)
    HIPCHK(e, hipStreamSynchronize(e->st));
    if (L.Op.regime && (rc0 = lg_union_clusters(e, {}, L.opt_cl, ucl))) return rc0;
    L.shift_bufs = LgShiftBufs{};
    L.Sh = LgShifts{};
    L.n_shift_cl = 0;
    L.shift_cl.clear();
    if (L.Op.regime) { L.n_disp_cl = (int32_t)L.opt_cl.size(); L.disp_cl = std::move(ucl); }
    return PGBP_OK;
  }
  // univariate per-site batches: the values once more as [shift][site], what the thread-per-site correction reads
  std::vector<double> vsm;
  if (per_site && L.T.uni_ok) {
    const size_t row = (size_t)sm_row(e->plan.n_sites);
    vsm.assign(n * row, 0.0);
    for (size_t s = 0; s < ns; ++s)
      for (size_t i = 0; i < n; ++i) vsm[i * row + s] = value[s * n + i];
  }
  LgShiftBufs B;
  int rc;
  if ((rc = dev_alloc(e, B.slot, slot.size()))) return rc;
  if ((rc = dev_alloc(e, B.cl, cl.size()))) return rc;
  if ((rc = dev_alloc(e, B.value, ns * n * pp))) return rc;
  if (!vsm.empty() && (rc = dev_alloc(e, B.value_sm, vsm.size()))) return rc;
  int32_t n_ucl = 0;
  if (L.Op.regime && (rc = lg_union_clusters(e, cl, L.opt_cl, ucl, &n_ucl))) return rc;
  // every buffer exists: the copies, then ONE synchronisation whatever they returned (none may outlive the host vectors)
  hipError_t herr = hipMemcpyAsync(B.slot.get(), slot.data(), slot.size() * sizeof(int32_t), hipMemcpyHostToDevice, e->st);
  if (herr == hipSuccess) herr = hipMemcpyAsync(B.cl.get(), cl.data(), cl.size() * sizeof(int32_t), hipMemcpyHostToDevice, e->st);
  if (herr == hipSuccess) herr = hipMemcpyAsync(B.value.get(), value, ns * n * pp * sizeof(double), hipMemcpyHostToDevice, e->st);
  if (herr == hipSuccess && !vsm.empty())
    herr = hipMemcpyAsync(B.value_sm.get(), vsm.data(), vsm.size() * sizeof(double), hipMemcpyHostToDevice, e->st);
  const hipError_t serr = hipStreamSynchronize(e->st);  // the host buffers may go away; kernels that read the old shifts have finished
  if (herr == hipSuccess) herr = serr;
  if (herr != hipSuccess) return e->fail(PGBP_ERR_HIP, std::string("pgbp_lg_set_shifts (upload): ") + hipGetErrorString(herr));
  L.shift_bufs = std::move(B);
  const LgShiftBufs& S = L.shift_bufs;
  L.Sh = LgShifts{S.slot.get(), S.value.get(), per_site ? 1 : 0, n_shifts, S.value_sm.get()};
  L.n_shift_cl = (int32_t)cl.size();
  L.shift_cl = std::move(cl);
  if (L.Op.regime) { L.n_disp_cl = n_ucl; L.disp_cl = std::move(ucl); }
  return PGBP_OK;
}

int32_t pgbp_lg_shift_count(pgbp_engine* e) {
  if (!e || !e->lg) return -1;
  return e->lg->Sh.slot ? e->lg->Sh.n : 0;
}

int pgbp_lg_set_optima(pgbp_engine* e, int32_t n_regimes, const int32_t* regime, const double* value, int32_t per_site) {
  DeviceScope device_scope(e);
  if (!e) return PGBP_ERR_INVALID;
  if (!e->lg) return e->fail(PGBP_ERR_STATE, "pgbp_lg_set_optima: no family table (call pgbp_lg_setup first)");
  LgModel& L = *e->lg;
  std::vector<int32_t> map, cl;   // the regime of every edge, and the clusters that hold a painted family, in index order
  std::string why;
  if (!L.T.optima_list(n_regimes, regime, value, per_site, map, cl, why)) return e->fail(PGBP_ERR_INVALID, why);
  if (n_regimes == 0) {   // clear (kernels already enqueued may still read the old optima)
    HIPCHK(e, hipStreamSynchronize(e->st));
    L.opt_bufs = LgOptimaBufs{};
    L.Op = LgOptima{};
    L.opt_cl.clear();
    L.disp_cl = DevBuf<int32_t>{};
    L.n_disp_cl = 0;
    return PGBP_OK;
  }
  const int pp = L.T.p;
  const size_t ns = per_site ? (size_t)e->plan.n_sites : 1, n = (size_t)n_regimes;
  // univariate per-site batches: the values once more as [regime][site], whole lines for lanes = sites
  std::vector<double> vsm;
  if (per_site && L.T.uni_ok) {
    const size_t row = (size_t)sm_row(e->plan.n_sites);
    vsm.assign(n * row, 0.0);
    for (size_t s = 0; s < ns; ++s)
      for (size_t i = 0; i < n; ++i) vsm[i * row + s] = value[s * n + i];
  }
  LgOptimaBufs B;
  DevBuf<int32_t> ucl;
  int32_t n_ucl = 0;
  int rc;
  if ((rc = dev_alloc(e, B.regime, map.size()))) return rc;
  if ((rc = dev_alloc(e, B.value, ns * n * pp))) return rc;
  if (!vsm.empty() && (rc = dev_alloc(e, B.value_sm, vsm.size()))) return rc;
  if ((rc = lg_union_clusters(e, L.shift_cl, cl, ucl, &n_ucl))) return rc;
  // every buffer exists: the copies, then ONE synchronisation whatever they returned (none may outlive the host vectors)
  hipError_t herr = hipMemcpyAsync(B.regime.get(), map.data(), map.size() * sizeof(int32_t), hipMemcpyHostToDevice, e->st);
  if (herr == hipSuccess) herr = hipMemcpyAsync(B.value.get(), value, ns * n * pp * sizeof(double), hipMemcpyHostToDevice, e->st);
  if (herr == hipSuccess && !vsm.empty())
    herr = hipMemcpyAsync(B.value_sm.get(), vsm.data(), vsm.size() * sizeof(double), hipMemcpyHostToDevice, e->st);
  const hipError_t serr = hipStreamSynchronize(e->st);  // the host buffers may go away; kernels that read the old optima have finished
  if (herr == hipSuccess) herr = serr;
  if (herr != hipSuccess) return e->fail(PGBP_ERR_HIP, std::string("pgbp_lg_set_optima (upload): ") + hipGetErrorString(herr));
  L.opt_bufs = std::move(B);
  const LgOptimaBufs& S = L.opt_bufs;
  L.Op = LgOptima{S.regime.get(), S.value.get(), per_site ? 1 : 0, n_regimes, S.value_sm.get()};
  L.opt_cl = std::move(cl);
  L.disp_cl = std::move(ucl);
  L.n_disp_cl = n_ucl;
  return PGBP_OK;
}

// The values alone, into the buffers of the setting in force: what a fit moves at every step.  The regime map, the cluster
// union and the buffers stay; every check before anything changes.
int pgbp_lg_update_optima(pgbp_engine* e, const double* value) {
  DeviceScope device_scope(e);
  if (!e) return PGBP_ERR_INVALID;
  if (!e->lg) return e->fail(PGBP_ERR_STATE, "pgbp_lg_update_optima: no family table (call pgbp_lg_setup first)");
  LgModel& L = *e->lg;
  if (!L.Op.regime) return e->fail(PGBP_ERR_STATE, "pgbp_lg_update_optima: no optima are set (call pgbp_lg_set_optima first)");
  if (!value) return e->fail(PGBP_ERR_INVALID, "pgbp_lg_update_optima: no values");
  const size_t ns = L.Op.per_site ? (size_t)e->plan.n_sites : 1, n = (size_t)L.Op.n, pp = (size_t)L.T.p;
  for (size_t i = 0; i < ns * n * pp; ++i)
    if (!std::isfinite(value[i]))
      return e->fail(PGBP_ERR_INVALID, "pgbp_lg_update_optima: value of regime " + std::to_string((i / pp) % n + 1) +
                                           (L.Op.per_site ? " at site " + std::to_string(i / (pp * n)) : std::string()) + ": trait " +
                                           std::to_string(i % pp) + " is not finite");
  std::vector<double> vsm;
  if (L.Op.value_sm) {   // (a univariate per-site batch: the [regime][site] rows as well)
    const size_t row = (size_t)sm_row(e->plan.n_sites);
    vsm.assign(n * row, 0.0);
    for (size_t s = 0; s < ns; ++s)
      for (size_t i = 0; i < n; ++i) vsm[i * row + s] = value[s * n + i];
  }
  hipError_t herr = hipStreamSynchronize(e->st);   // kernels that read the old values have finished
  if (herr == hipSuccess) herr = hipMemcpyAsync(L.opt_bufs.value.get(), value, ns * n * pp * sizeof(double), hipMemcpyHostToDevice, e->st);
  if (herr == hipSuccess && !vsm.empty())
    herr = hipMemcpyAsync(L.opt_bufs.value_sm.get(), vsm.data(), vsm.size() * sizeof(double), hipMemcpyHostToDevice, e->st);
  const hipError_t serr = hipStreamSynchronize(e->st);   // the host buffers may go away
  if (herr == hipSuccess) herr = serr;
  if (herr != hipSuccess) return e->fail(PGBP_ERR_HIP, std::string("pgbp_lg_update_optima (upload): ") + hipGetErrorString(herr));
  return PGBP_OK;
}

int32_t pgbp_lg_optima_count(pgbp_engine* e) {
  if (!e || !e->lg) return -1;
  return e->lg->Op.regime ? e->lg->Op.n : 0;
}

int pgbp_lg_set_tip_noise(pgbp_engine* e, int32_t n, const int32_t* family, const double* scale, const double* sigma_e,
                          const double* se2, int32_t per_site) {
  DeviceScope device_scope(e);
  if (!e) return PGBP_ERR_INVALID;
  if (!e->lg) return e->fail(PGBP_ERR_STATE, "pgbp_lg_set_tip_noise: no family table (call pgbp_lg_setup first)");
  LgModel& L = *e->lg;
  // the slot table, sigma_e exactly symmetric, the clusters that hold a noisy tip family, in index order, and what the
  // correction kernel needs for the largest of them
  std::vector<int32_t> slot, cl;
  std::vector<double> sig;
  int32_t max_dim = 0;
  std::string why;
  if (!L.T.noise_list(n, family, scale, sigma_e, se2, per_site, slot, sig, cl, &max_dim, why)) return e->fail(PGBP_ERR_INVALID, why);
  const int pp = L.T.p, K = L.T.K;
  const size_t ns = per_site ? (size_t)e->plan.n_sites : 1, nn = (size_t)n;
  if (n > 0) {
    const size_t bytes = lg_noise_lds_bytes(pp, K, max_dim);
    if (bytes > 160 * 1024)
      return e->fail(PGBP_ERR_INVALID, "pgbp_lg_set_tip_noise: a cluster of " + std::to_string(max_dim) + " variables with " +
                                           std::to_string(pp) + " traits holds a noisy tip; its correction needs " +
                                           std::to_string(bytes) + " bytes of LDS, more than the 160 KB of a compute unit");
  }
  if (n == 0) {   // clear (kernels already enqueued may still read the old noise)
    HIPCHK(e, hipStreamSynchronize(e->st));
    L.noise_bufs = LgNoiseBufs{};
    L.Nz = LgNoise{};
    L.n_noise_cl = L.noise_max_dim = 0;
    return PGBP_OK;
  }
  // univariate per-site batches: se2 once more as [slot][site], what the thread-per-site correction reads
  std::vector<double> ssm;
  if (per_site && se2 && L.T.uni_ok) {
    const size_t row = (size_t)sm_row(e->plan.n_sites);
    ssm.assign(nn * row, 0.0);
    for (size_t s = 0; s < ns; ++s)
      for (size_t i = 0; i < nn; ++i) ssm[i * row + s] = se2[s * nn + i];
  }
  LgNoiseBufs B;
  int rc;
  if ((rc = dev_alloc(e, B.slot, slot.size()))) return rc;
  if ((rc = dev_alloc(e, B.cl, cl.size()))) return rc;
  if ((rc = dev_alloc(e, B.scale, nn))) return rc;
  if ((rc = dev_alloc(e, B.sigma_e, sig.size()))) return rc;
  if (se2 && (rc = dev_alloc(e, B.se2, ns * nn * pp))) return rc;
  if (!ssm.empty() && (rc = dev_alloc(e, B.se2_sm, ssm.size()))) return rc;
  // every buffer exists: the copies, then ONE synchronisation whatever they returned (none may outlive the host vectors)
  hipError_t herr = hipMemcpyAsync(B.slot.get(), slot.data(), slot.size() * sizeof(int32_t), hipMemcpyHostToDevice, e->st);
  if (herr == hipSuccess) herr = hipMemcpyAsync(B.cl.get(), cl.data(), cl.size() * sizeof(int32_t), hipMemcpyHostToDevice, e->st);
  if (herr == hipSuccess) herr = hipMemcpyAsync(B.scale.get(), scale, nn * sizeof(double), hipMemcpyHostToDevice, e->st);
  if (herr == hipSuccess) herr = hipMemcpyAsync(B.sigma_e.get(), sig.data(), sig.size() * sizeof(double), hipMemcpyHostToDevice, e->st);
  if (herr == hipSuccess && se2)
    herr = hipMemcpyAsync(B.se2.get(), se2, ns * nn * pp * sizeof(double), hipMemcpyHostToDevice, e->st);
  if (herr == hipSuccess && !ssm.empty())
    herr = hipMemcpyAsync(B.se2_sm.get(), ssm.data(), ssm.size() * sizeof(double), hipMemcpyHostToDevice, e->st);
  const hipError_t serr = hipStreamSynchronize(e->st);  // the host buffers may go away; kernels that read the old noise have finished
  if (herr == hipSuccess) herr = serr;
  if (herr != hipSuccess) return e->fail(PGBP_ERR_HIP, std::string("pgbp_lg_set_tip_noise (upload): ") + hipGetErrorString(herr));
  L.noise_bufs = std::move(B);
  const LgNoiseBufs& S = L.noise_bufs;
  L.Nz = LgNoise{S.slot.get(), S.scale.get(), S.sigma_e.get(), se2 ? S.se2.get() : nullptr, per_site ? 1 : 0, n, S.se2_sm.get()};
  L.n_noise_cl = (int32_t)cl.size();
  L.noise_max_dim = max_dim;
  return PGBP_OK;
}

int32_t pgbp_lg_tip_noise_count(pgbp_engine* e) {
  if (!e || !e->lg) return -1;
  return e->lg->Nz.slot ? e->lg->Nz.n : 0;
}

int pgbp_lg_set_site_missing(pgbp_engine* e, const uint8_t* missing) {
  DeviceScope device_scope(e);
  if (!e) return PGBP_ERR_INVALID;
  const char* fn = "pgbp_lg_set_site_missing";
  if (!e->lg) return e->fail(PGBP_ERR_STATE, std::string(fn) + ": no family table (call pgbp_lg_setup first)");
  LgModel& L = *e->lg;
  if (!missing) {   // clear, on any engine with a table (kernels already enqueued may still read the old mask)
    HIPCHK(e, hipStreamSynchronize(e->st));
    L.miss_bufs = LgSiteMissBufs{};
    L.Ms = LgSiteMiss{};
    L.miss = SiteMissPack{};
    return PGBP_OK;
  }
  // a thread-per-site engine, as the lanes-are-sites sweeps define it (pgbp_sites_host.hpp)
  const SitesCall c{&L, engine_peek(e), engine_uni_view(e), 0};
  int rc = sites_accept_engine(e, fn, "pgbp_patterns: one engine per missingness pattern", c);
  if (rc) return rc;
  const LgTable& T = L.T;
  const SiteMissTable tab{e->plan.n_sites, T.n_rows, T.n_families, T.cluster.data(), T.data_row.data(), T.tip.data(),
                          T.child_mask.empty() ? nullptr : T.child_mask.data()};
  SiteMissPack P;
  std::string why;
  if (!site_missing_pack(tab, missing, P, why)) return e->fail(PGBP_ERR_INVALID, why);
  if (P.count == 0) return pgbp_lg_set_site_missing(e, nullptr);   // nothing is masked: no mask, nothing is launched
  LgSiteMissBufs B;
  if ((rc = dev_alloc(e, B.words, P.words.size()))) return rc;
  if ((rc = dev_alloc(e, B.cl, P.cl.size()))) return rc;
  // every buffer exists: the copies, the 0.0 at the masked entries of both copies of the data, then ONE synchronisation
  hipError_t herr = hipMemcpyAsync(B.words.get(), P.words.data(), P.words.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, e->st);
  if (herr == hipSuccess) herr = hipMemcpyAsync(B.cl.get(), P.cl.data(), P.cl.size() * sizeof(int32_t), hipMemcpyHostToDevice, e->st);
  const LgSiteMiss Ms{B.words.get(), P.W};
  if (herr == hipSuccess) {
    launch_lg_sitemiss_zero(Ms, L.bufs.data.get(), L.bufs.data_sm.get(), T.n_rows, e->plan.n_sites, e->st);
    herr = hipGetLastError();
  }
  const hipError_t serr = hipStreamSynchronize(e->st);  // the host buffers may go away; kernels that read the old mask have finished
  if (herr == hipSuccess) herr = serr;
  if (herr != hipSuccess) return e->fail(PGBP_ERR_HIP, std::string(fn) + " (upload): " + hipGetErrorString(herr));
  L.miss_bufs = std::move(B);
  L.Ms = Ms;
  L.miss = std::move(P);
  return PGBP_OK;
}

int pgbp_lg_get_site_missing(pgbp_engine* e, uint8_t* missing) {
  if (!e) return PGBP_ERR_INVALID;
  if (!e->lg) return e->fail(PGBP_ERR_STATE, "pgbp_lg_get_site_missing: no family table (call pgbp_lg_setup first)");
  if (!missing) return e->fail(PGBP_ERR_INVALID, "pgbp_lg_get_site_missing: no buffer");
  site_missing_unpack(e->lg->miss, e->plan.n_sites, e->lg->T.n_rows, missing);
  return PGBP_OK;
}

int32_t pgbp_lg_site_missing_count(pgbp_engine* e) {
  if (!e || !e->lg) return -1;
  return e->lg->Ms.words ? (int32_t)std::min<int64_t>(e->lg->miss.count, INT32_MAX) : 0;
}

// Per-site clade shifts of the optimum: every check (pgbp_cladeshift_host.hpp) before anything changes; new buffers into a local
// group that the model takes once every copy has been made.  Rows [slot][site] padded to sm_row in both layouts, the padding
// and the empty slots at family -1 and delta 0.
static void clade_rows(int32_t n_slots, int n_sites, const int32_t* family, const double* delta, std::vector<int32_t>* fr,
                       std::vector<double>& dr) {
  const size_t row = (size_t)sm_row(n_sites), ns = (size_t)n_sites;
  if (fr) fr->assign((size_t)n_slots * row, -1);
  dr.assign((size_t)n_slots * row, 0.0);
  for (size_t j = 0; j < (size_t)n_slots; ++j)
    for (size_t s = 0; s < ns; ++s) {
      const int32_t v = family[j * ns + s];
      if (fr) (*fr)[j * row + s] = v;
      dr[j * row + s] = v >= 0 ? delta[j * ns + s] : 0.0;
    }
}

int pgbp_lg_set_clade_shifts_sites(pgbp_engine* e, int32_t n_slots, const int32_t* family, const double* delta) {
  DeviceScope device_scope(e);
  if (!e) return PGBP_ERR_INVALID;
  const char* fn = "pgbp_lg_set_clade_shifts_sites";
  if (!e->lg) return e->fail(PGBP_ERR_STATE, std::string(fn) + ": no family table (call pgbp_lg_setup first)");
  LgModel& L = *e->lg;
  if (n_slots < 0) return e->fail(PGBP_ERR_INVALID, std::string(fn) + ": negative number of slots");
  if (n_slots == 0) {   // clear, on any engine with a table (kernels already enqueued may still read the old setting)
    HIPCHK(e, hipStreamSynchronize(e->st));
    L.clade_bufs = LgCladeBufs{};
    L.Cs = LgCladeShifts{};
    L.clade_family.clear();
    L.clade_delta.clear();
    L.n_clade_cl = 0;
    return PGBP_OK;
  }
  // a thread-per-site engine, as the lanes-are-sites sweeps define it (pgbp_sites_host.hpp)
  const SitesCall c{&L, engine_peek(e), engine_uni_view(e), 0};
  int rc = sites_accept_engine(e, fn, "pgbp_lg_set_optima: one regime map for all sites", c);
  if (rc) return rc;
  if (!L.clade.built) return e->fail(PGBP_ERR_STATE, std::string(fn) + ": no topology (call pgbp_lg_set_topology first)");
  std::string why;
  if (!optscan_plan_single_parents(L.optscan, L.T.n_parents.data(), why)) return e->fail(PGBP_ERR_INVALID, std::string(fn) + ": " + why);
  const int n_sites = e->plan.n_sites;
  if (!clade_setting_check(L.clade, L.T.n_parents.data(), n_slots, n_sites, family, delta, why))
    return e->fail(PGBP_ERR_INVALID, std::string(fn) + ": " + why);
  std::vector<int32_t> cl, fr;
  std::vector<double> dr;
  clade_clusters(L.clade, L.T.cluster.data(), n_slots, n_sites, family, cl);
  const int32_t n_cl = (int32_t)cl.size();
  if (cl.empty()) cl.push_back(0);
  clade_rows(n_slots, n_sites, family, delta, &fr, dr);
  LgCladeBufs B;
  if ((rc = dev_alloc(e, B.family, fr.size()))) return rc;
  if ((rc = dev_alloc(e, B.delta, dr.size()))) return rc;
  if ((rc = dev_alloc(e, B.cl, cl.size()))) return rc;
  // every buffer exists: the copies, then ONE synchronisation whatever they returned (none may outlive the host vectors)
  hipError_t herr = hipMemcpyAsync(B.family.get(), fr.data(), fr.size() * sizeof(int32_t), hipMemcpyHostToDevice, e->st);
  if (herr == hipSuccess) herr = hipMemcpyAsync(B.delta.get(), dr.data(), dr.size() * sizeof(double), hipMemcpyHostToDevice, e->st);
  if (herr == hipSuccess) herr = hipMemcpyAsync(B.cl.get(), cl.data(), cl.size() * sizeof(int32_t), hipMemcpyHostToDevice, e->st);
  const hipError_t serr = hipStreamSynchronize(e->st);  // the host buffers may go away; kernels that read the old setting have finished
  if (herr == hipSuccess) herr = serr;
  if (herr != hipSuccess) return e->fail(PGBP_ERR_HIP, std::string(fn) + " (upload): " + hipGetErrorString(herr));
  L.clade_bufs = std::move(B);
  L.Cs = LgCladeShifts{L.clade_bufs.family.get(), L.clade_bufs.delta.get(), L.d_clade_pre.get(), L.d_clade_last.get(), n_slots,
                       sm_row(n_sites)};
  const size_t n = (size_t)n_slots * (size_t)n_sites;
  L.clade_family.assign(family, family + n);
  L.clade_delta.assign(delta, delta + n);
  for (size_t i = 0; i < n; ++i)
    if (family[i] < 0) L.clade_delta[i] = 0.0;
  L.n_clade_cl = n_cl;
  return PGBP_OK;
}

// The values alone, into the buffers of the setting in force: what a refit moves at every step.  The families, the cluster list
// and the buffers stay; every check before anything changes.
int pgbp_lg_update_clade_shifts_sites(pgbp_engine* e, const double* delta) {
  DeviceScope device_scope(e);
  if (!e) return PGBP_ERR_INVALID;
  const char* fn = "pgbp_lg_update_clade_shifts_sites";
  if (!e->lg) return e->fail(PGBP_ERR_STATE, std::string(fn) + ": no family table (call pgbp_lg_setup first)");
  LgModel& L = *e->lg;
  if (!L.Cs.family) return e->fail(PGBP_ERR_STATE, std::string(fn) + ": no clade shifts are set (call pgbp_lg_set_clade_shifts_sites first)");
  const int n_sites = e->plan.n_sites;
  std::string why;
  if (!clade_values_check(L.Cs.n_slots, n_sites, L.clade_family.data(), delta, why))
    return e->fail(PGBP_ERR_INVALID, std::string(fn) + ": " + why);
  std::vector<double> dr;
  clade_rows(L.Cs.n_slots, n_sites, L.clade_family.data(), delta, nullptr, dr);
  hipError_t herr = hipStreamSynchronize(e->st);   // kernels that read the old values have finished
  if (herr == hipSuccess) herr = hipMemcpyAsync(L.clade_bufs.delta.get(), dr.data(), dr.size() * sizeof(double), hipMemcpyHostToDevice, e->st);
  const hipError_t serr = hipStreamSynchronize(e->st);   // the host buffer may go away
  if (herr == hipSuccess) herr = serr;
  if (herr != hipSuccess) return e->fail(PGBP_ERR_HIP, std::string(fn) + " (upload): " + hipGetErrorString(herr));
  const size_t n = (size_t)L.Cs.n_slots * (size_t)n_sites;
  for (size_t i = 0; i < n; ++i) L.clade_delta[i] = L.clade_family[i] >= 0 ? delta[i] : 0.0;
  return PGBP_OK;
}

int32_t pgbp_lg_clade_shift_slots(pgbp_engine* e) {
  if (!e || !e->lg) return -1;
  return e->lg->Cs.family ? e->lg->Cs.n_slots : 0;
}

int pgbp_lg_get_clade_shifts_sites(pgbp_engine* e, int32_t* family, double* delta) {
  if (!e) return PGBP_ERR_INVALID;
  if (!e->lg) return e->fail(PGBP_ERR_STATE, "pgbp_lg_get_clade_shifts_sites: no family table (call pgbp_lg_setup first)");
  const LgModel& L = *e->lg;
  if (family) std::copy(L.clade_family.begin(), L.clade_family.end(), family);
  if (delta) std::copy(L.clade_delta.begin(), L.clade_delta.end(), delta);
  return PGBP_OK;
}

int pgbp_lg_set_topology(pgbp_engine* e, const int32_t* parent_family) {
  DeviceScope device_scope(e);
  if (!e) return PGBP_ERR_INVALID;
  if (!e->lg) return e->fail(PGBP_ERR_STATE, "pgbp_lg_set_topology: no family table (call pgbp_lg_setup first)");
  LgModel& L = *e->lg;
  const int K = L.T.K, nf = L.T.n_families;
  if (nf > 0 && !parent_family) return e->fail(PGBP_ERR_INVALID, "pgbp_lg_set_topology: no table");
  std::vector<int32_t> level_off, level_fam;
  int32_t improper = -1;
  std::string why;
  if (!lg_topology_levels(nf, K, L.T.n_parents.data(), parent_family, level_off, level_fam, &improper, why))
    return e->fail(PGBP_ERR_INVALID, "pgbp_lg_set_topology: " + why);
  std::vector<int32_t> pf(std::max<size_t>(1, (size_t)nf * K), kTopoFixedRoot);
  for (int f = 0; f < nf; ++f)
    for (int k = 0; k < L.T.n_parents[f]; ++k) pf[(size_t)f * K + k] = parent_family[(size_t)f * K + k];
  if (level_fam.empty()) level_fam.push_back(0);
  // the plan of the optimum-shift scan: child lists, heights (a network is accepted here and refused by the scan)
  OptScanPlan os;
  if (!optscan_plan_build(nf, K, L.T.n_parents.data(), parent_family, os, why))
    return e->fail(PGBP_ERR_INVALID, "pgbp_lg_set_topology: " + why);
  // the preorder ranks of the family tree: membership in a clade for pgbp_lg_set_clade_shifts_sites
  CladePlan cp;
  if (!clade_plan_build(nf, K, L.T.n_parents.data(), parent_family, cp, why))
    return e->fail(PGBP_ERR_INVALID, "pgbp_lg_set_topology: " + why);
  std::vector<int32_t> cp_pre = cp.pre, cp_last = cp.last;
  if (cp_pre.empty()) { cp_pre.push_back(0); cp_last.push_back(0); }
  std::vector<int32_t> os_cf = os.child_fam, os_hf = os.height_fam;
  if (os_cf.empty()) os_cf.push_back(0);
  if (os_hf.empty()) os_hf.push_back(0);
  DevBuf<int32_t> d_pf, d_lf, d_co, d_cf, d_hf, d_cpre, d_clast;
  int rc;
  if ((rc = upload(e, d_cpre, cp_pre))) return rc;
  if ((rc = upload(e, d_clast, cp_last))) return rc;
  if ((rc = upload(e, d_pf, pf))) return rc;
  if ((rc = upload(e, d_lf, level_fam))) return rc;
  if ((rc = upload(e, d_co, os.child_off))) return rc;
  if ((rc = upload(e, d_cf, os_cf))) return rc;
  if ((rc = upload(e, d_hf, os_hf))) return rc;
  // a setting of clade shifts names families by the ranks of the topology it was checked against: a new one clears it
  HIPCHK(e, hipStreamSynchronize(e->st));
  L.clade_bufs = LgCladeBufs{};
  L.Cs = LgCladeShifts{};
  L.clade_family.clear();
  L.clade_delta.clear();
  L.n_clade_cl = 0;
  L.clade = std::move(cp);
  L.d_clade_pre = std::move(d_cpre);
  L.d_clade_last = std::move(d_clast);
  L.optscan = std::move(os);
  L.d_os_child_off = std::move(d_co);
  L.d_os_child_fam = std::move(d_cf);
  L.d_os_height_fam = std::move(d_hf);
  L.d_pf = std::move(d_pf);
  L.d_level_fam = std::move(d_lf);
  L.level_off = std::move(level_off);
  L.improper = improper;
  return PGBP_OK;
}

// the table, then its checks of the range and, where it says observed, of the values of sites [site_begin, site_end)
static int lg_check_data(pgbp_engine* e, const char* fn, int32_t site_begin, int32_t site_end, const double* data, bool values) {
  if (!e->lg) return e->fail(PGBP_ERR_STATE, std::string(fn) + ": no family table (call pgbp_lg_setup first)");
  std::string why;
  if (!e->lg->T.check_data(fn, site_begin, site_end, data, values, why, e->lg->Ms.words ? &e->lg->miss : nullptr))
    return e->fail(PGBP_ERR_INVALID, why);
  return PGBP_OK;
}

int pgbp_lg_set_data(pgbp_engine* e, int32_t site_begin, int32_t site_end, const double* data) {
  DeviceScope device_scope(e);
  if (!e) return PGBP_ERR_INVALID;
  const int rc = lg_check_data(e, "pgbp_lg_set_data", site_begin, site_end, data, true);
  if (rc) return rc;
  const LgModel& L = *e->lg;
  const size_t per = (size_t)L.T.n_rows * L.T.p, n = (size_t)(site_end - site_begin) * per;
  if (n == 0) return PGBP_OK;
  double* dst = L.bufs.data.get() + (size_t)site_begin * per;
  std::vector<double> clean;   // as the set-up: masked-out entries may be NaN on the host, they never reach arithmetic
  if (!L.T.child_mask.empty() || L.Ms.words) {
    clean.assign(data, data + n);
    for (double& x : clean) if (!std::isfinite(x)) x = 0.0;
    if (L.Ms.words)   // a per-site mask in force: 0.0 at its entries, whatever was given
      for (int32_t s = site_begin; s < site_end; ++s)
        for (int32_t r = 0; r < L.T.n_rows; ++r)
          if (site_missing_test(L.miss, r, s)) clean[(size_t)(s - site_begin) * per + r] = 0.0;
    data = clean.data();
  }
  hipError_t herr = hipMemcpyAsync(dst, data, n * sizeof(double), hipMemcpyHostToDevice, e->st);
  if (herr == hipSuccess && L.bufs.data_sm)   // the [row][site] copy of a univariate batch, whole
    launch_transpose_words_f64(L.bufs.data.get(), L.bufs.data_sm.get(), L.T.n_rows, e->plan.n_sites, 1, e->st);
  const hipError_t serr = hipStreamSynchronize(e->st);  // the host buffers may go away
  if (herr == hipSuccess) herr = serr;
  if (herr != hipSuccess) return e->fail(PGBP_ERR_HIP, std::string("pgbp_lg_set_data (upload): ") + hipGetErrorString(herr));
  return PGBP_OK;
}

int pgbp_lg_get_data(pgbp_engine* e, int32_t site_begin, int32_t site_end, double* data) {
  DeviceScope device_scope(e);
  if (!e) return PGBP_ERR_INVALID;
  const int rc = lg_check_data(e, "pgbp_lg_get_data", site_begin, site_end, data, false);
  if (rc) return rc;
  const LgModel& L = *e->lg;
  const size_t per = (size_t)L.T.n_rows * L.T.p, n = (size_t)(site_end - site_begin) * per;
  if (n == 0) return PGBP_OK;
  HIPCHK(e, hipMemcpyAsync(data, L.bufs.data.get() + (size_t)site_begin * per, n * sizeof(double), hipMemcpyDeviceToHost, e->st));
  HIPCHK(e, hipStreamSynchronize(e->st));
  return PGBP_OK;
}

int pgbp_enqueue_loglik_lg(pgbp_engine* e, int32_t reps, const pgbp_opts* opts) {
  DeviceScope device_scope(e);
  if (!e) return PGBP_ERR_INVALID;
  int rc = check_opts(e, opts);
  if (rc) return rc;
  if ((rc = need_schedule(e, 0))) return rc;
  if (!e->lg || !e->lg->have_params)
    return e->fail(PGBP_ERR_STATE, "pgbp_enqueue_loglik_lg: call pgbp_lg_setup / pgbp_lg_assignfactors first");
  if ((rc = reset_fail(e))) return rc;
  if ((rc = ensure_layout(e, want_bs16(e), want_site_minor(e)))) return rc;
  DevState S = dev_state(e, opts);
  const Plan& p = e->plan;
  for (int r = 0; r < reps; ++r) {
    DevState S1 = S;
    S1.sep_zero = fresh_sepsets_shortcut(e) ? 1 : 0;
    if ((rc = lg_fill_async(e, false, S1.sep_zero != 0))) return rc;  // assignfactors!        calibration.jl:205-209
    enqueue_tree(e, S1, 0, 1, 0);                                     // postorder             :210
    const int root = p.trees[0].pa.empty() ? 0 : p.trees[0].pa[0];
    integrate_async(e, root, nullptr);                                // :212
  }
  return e->take_enqueue_rc();
}

// ---- benchmarking / zero-copy entry points ---------------------------------------------------

// one iteration of calibrate! over every schedule tree.  ev != null: one HIP event pair around the message launches of
// each tree (they run back to back on the stream), *n_launches += their number
static int enqueue_calibrate_once(pgbp_engine* e, const DevState& S, int reset_each, std::vector<EventPair>* ev,
                                  int* n_launches = nullptr) {
  const Plan& p = e->plan;
  if (reset_each) {
    int rc = reset_from_factors_async(e);
    if (rc) return rc;
    reset_message_flags(e, 1);
  }
  for (int j = 0; j < (int)p.trees.size(); ++j) {
    EventPair pr;
    if (ev) {
      HIPCHK(e, hipError_t(pr.create()));
      HIPCHK(e, hipEventRecord(hip_event(pr.first()), e->st));
    }
    enqueue_pair_and_iscal(e, S, j, (unsigned long long)j, false, e->d_iscal.get(), n_launches);
    if (ev) {
      HIPCHK(e, hipEventRecord(hip_event(pr.second()), e->st));
      ev->push_back(std::move(pr));
    }
  }
  return PGBP_OK;
}

int pgbp_enqueue_calibrate(pgbp_engine* e, int32_t reps, int32_t reset_each, const pgbp_opts* opts) {
  DeviceScope device_scope(e);
  if (!e) return PGBP_ERR_INVALID;
  int rc = check_opts(e, opts);
  if (rc) return rc;
  if ((rc = need_schedule(e, 0))) return rc;
  if ((rc = reset_fail(e))) return rc;
  if ((rc = ensure_layout(e, want_bs16(e), want_site_minor(e)))) return rc;
  DevState S = dev_state(e, opts);
  for (int r = 0; r < reps; ++r)
    if ((rc = enqueue_calibrate_once(e, S, reset_each, nullptr))) return rc;
  return e->take_enqueue_rc();
}

static void drop_kernel_events(pgbp_engine* e) {
  e->kernel_events.clear();
  e->kernel_launches = 0;
}

int pgbp_enqueue_calibrate_timed(pgbp_engine* e, int32_t reps, int32_t reset_each, const pgbp_opts* opts) {
  DeviceScope device_scope(e);
  if (!e) return PGBP_ERR_INVALID;
  int rc = check_opts(e, opts);
  if (rc) return rc;
  if ((rc = need_schedule(e, 0))) return rc;
  if ((rc = reset_fail(e))) return rc;
  if ((rc = ensure_layout(e, want_bs16(e), want_site_minor(e)))) return rc;
  drop_kernel_events(e);
  DevState S = dev_state(e, opts);
  int launches = 0;
  if (reset_each) {
    // resets between the repetitions: an event pair around the message launches of every schedule tree
    for (int r = 0; r < reps; ++r)
      if ((rc = enqueue_calibrate_once(e, S, reset_each, &e->kernel_events, &launches))) return rc;
  } else {
    // nothing but message launches (and the flag reduction behind each tree) in the region: ONE pair around all of it
    // -- an event record is a barrier packet on the stream, and two of them per repetition cost 4 % of a cfg3 calibrate
    EventPair pr;
    HIPCHK(e, hipError_t(pr.create()));
    const hipEvent_t a = hip_event(pr.first()), b = hip_event(pr.second());
    e->kernel_events.push_back(std::move(pr));
    HIPCHK(e, hipEventRecord(a, e->st));
    for (int r = 0; r < reps; ++r)
      if ((rc = enqueue_calibrate_once(e, S, 0, nullptr, &launches))) return rc;
    HIPCHK(e, hipEventRecord(b, e->st));
  }
  e->kernel_launches = launches;
  return e->take_enqueue_rc();
}

int pgbp_fetch_kernel_time(pgbp_engine* e, float* ms_kernels, int32_t* n_launches) {
  DeviceScope device_scope(e);
  if (!e || !ms_kernels) return PGBP_ERR_INVALID;
  HIPCHK(e, hipStreamSynchronize(e->st));
  HIPCHK(e, hipGetLastError());
  double total = 0;
  for (auto& pr : e->kernel_events) {
    float ms = 0;
    HIPCHK(e, hipEventElapsedTime(&ms, hip_event(pr.first()), hip_event(pr.second())));
    total += ms;
  }
  *ms_kernels = (float)total;
  if (n_launches) *n_launches = e->kernel_launches;
  drop_kernel_events(e);
  return PGBP_OK;
}

static int enqueue_loglik_once(pgbp_engine* e, const DevState& S0) {
  const Plan& p = e->plan;
  DevState S = S0;
  S.sep_zero = fresh_sepsets_shortcut(e) ? 1 : 0;
  int rc = reset_from_factors_async(e, S.sep_zero != 0);
  if (rc) return rc;
  reset_message_flags(e, 1);  // calibration.jl:209
  enqueue_tree(e, S, 0, 1, 0);                                                              // :210
  const int root = p.trees[0].pa.empty() ? 0 : p.trees[0].pa[0];
  integrate_async(e, root, nullptr);         // :212
  return PGBP_OK;
}

int pgbp_enqueue_loglik(pgbp_engine* e, int32_t reps, const pgbp_opts* opts) {
  DeviceScope device_scope(e);
  if (!e) return PGBP_ERR_INVALID;
  int rc = check_opts(e, opts);
  if (rc) return rc;
  if ((rc = need_schedule(e, 0))) return rc;
  if ((rc = reset_fail(e))) return rc;
  if ((rc = ensure_layout(e, want_bs16(e), want_site_minor(e)))) return rc;
  DevState S = dev_state(e, opts);
  for (int r = 0; r < reps; ++r)
    if ((rc = enqueue_loglik_once(e, S))) return rc;
  return e->take_enqueue_rc();
}

int32_t pgbp_layout(const pgbp_engine* e) { return e ? (e->layout_bs16 ? 1 : 0) | (e->layout_sm ? 2 : 0) : -1; }

int pgbp_enqueue_integrate(pgbp_engine* e, int32_t belief) {
  DeviceScope device_scope(e);
  if (!e) return PGBP_ERR_INVALID;
  if (belief < 0 || belief >= e->plan.n_beliefs()) return e->fail(PGBP_ERR_INVALID, "belief index out of range");
  integrate_async(e, belief, nullptr);
  return e->take_enqueue_rc();
}

int pgbp_fetch_loglik(pgbp_engine* e, double* norm, int32_t* info) {
  DeviceScope device_scope(e);
  if (!e || !norm) return PGBP_ERR_INVALID;
  const int ns = e->plan.n_sites;
  HIPCHK(e, hipMemcpyAsync(norm, e->d_norm.get(), sizeof(double) * ns, hipMemcpyDeviceToHost, e->st));
  if (info) HIPCHK(e, hipMemcpyAsync(info, e->d_info.get(), sizeof(int32_t) * ns, hipMemcpyDeviceToHost, e->st));
  HIPCHK(e, hipStreamSynchronize(e->st));
  HIPCHK(e, hipGetLastError());
  if (const int erc = e->take_enqueue_rc()) return erc;
  if (info) {
    // a failed postorder message also invalidates the likelihood
    std::vector<unsigned long long> keys(ns);
    HIPCHK(e, hipMemcpy(keys.data(), e->d_fail.get(), sizeof(unsigned long long) * ns, hipMemcpyDeviceToHost));
    for (int s = 0; s < ns; ++s)
      if (is_failure_key(keys[s]) && info[s] == 0) info[s] = (int32_t)(keys[s] & ((1ull << kInfoBits) - 1));
  }
  return PGBP_OK;
}

int pgbp_time_enqueued(pgbp_engine* e, int32_t kind, int32_t reps, int32_t reset_each, const pgbp_opts* opts,
                       float* ms_total) {
  DeviceScope device_scope(e);
  if (!e || !ms_total || kind < 0 || kind > 3) return PGBP_ERR_INVALID;
  EventPair pr;
  HIPCHK(e, hipError_t(pr.create()));
  const hipEvent_t a = hip_event(pr.first()), b = hip_event(pr.second());
  HIPCHK(e, hipStreamSynchronize(e->st));
  HIPCHK(e, hipEventRecord(a, e->st));
  int rc = kind == 0 ? pgbp_enqueue_calibrate(e, reps, reset_each, opts)
                     : (kind == 3 ? pgbp_enqueue_loglik_lg(e, reps, opts)
                                  : (kind == 2 ? pgbp_enqueue_loglik_bm(e, reps, opts) : pgbp_enqueue_loglik(e, reps, opts)));
  if (rc == PGBP_OK) {
    HIPCHK(e, hipEventRecord(b, e->st));
    HIPCHK(e, hipEventSynchronize(b));
    HIPCHK(e, hipEventElapsedTime(ms_total, a, b));
  }
  return rc;
}

int pgbp_time_message_kernels(pgbp_engine* e, int32_t reps, const pgbp_opts* opts, float* ms_kernels,
                              int32_t* n_launches) {
  DeviceScope device_scope(e);
  if (!e || !ms_kernels) return PGBP_ERR_INVALID;
  int rc = pgbp_enqueue_calibrate_timed(e, reps, 1, opts);
  if (rc) return rc;
  return pgbp_fetch_kernel_time(e, ms_kernels, n_launches);
}

int pgbp_traffic_model(const pgbp_engine* e, double* bytes_per_calibrate, int64_t* messages_per_calibrate) {
  if (!e) return PGBP_ERR_INVALID;
  int64_t nm = 0;
  double b = plan_bytes_per_calibrate(e->plan, &nm);
  if (bytes_per_calibrate) *bytes_per_calibrate = b;
  if (messages_per_calibrate) *messages_per_calibrate = nm;
  return PGBP_OK;
}

}  // extern "C"

// ---- internal (pgbp_dist.hip): one rank's contribution to the all-gather of pgbp_comm_gather_loglik -----------------------
namespace {
__global__ void pack_gather_slot(const double* __restrict__ norm, const int32_t* __restrict__ info,
                                 const unsigned long long* __restrict__ fail, const int32_t* __restrict__ iscal, int ns,
                                 int slot_sites, double* __restrict__ out) {
  // out[0 .. slot): log-likelihoods; out[slot .. 2 slot): info words; out[2 slot], out[2 slot + 1]: min over this rank's
  // sites of succ (no failed message) and iscal.  One workgroup.
  __shared__ int s_succ, s_iscal;
  if (threadIdx.x == 0) { s_succ = 1; s_iscal = 1; }
  __syncthreads();
  for (int i = threadIdx.x; i < slot_sites; i += blockDim.x) {
    const bool in = i < ns;
    const bool failed = in && pgbp::is_failure_key(fail[i]);
    out[i] = in ? norm[i] : 0.0;
    out[slot_sites + i] = in ? (double)(failed && info[i] == 0 ? (int)(fail[i] & ((1ull << pgbp::kInfoBits) - 1)) : info[i]) : 0.0;
    if (failed) atomicMin(&s_succ, 0);
    if (in && iscal[i] == 0) atomicMin(&s_iscal, 0);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    out[2 * slot_sites] = (double)s_succ;
    out[2 * slot_sites + 1] = (double)s_iscal;
  }
}
}  // namespace

namespace pgbp {
int engine_pack_gather_slot(pgbp_engine* e, int32_t slot_sites, double** d_slot, hipStream_t* st, int32_t* n_sites) {
  if (!e || !d_slot || !st) return PGBP_ERR_INVALID;
  DeviceScope device_scope(e);
  const int ns = e->plan.n_sites;
  if (slot_sites < ns) return e->fail(PGBP_ERR_INVALID, "gather slot smaller than this rank's number of sites");
  const int64_t need = 2 * (int64_t)slot_sites + 2;
  if (need > e->gather_cap) {
    e->gather_cap = 0;
    int rc = dev_alloc(e, e->d_gather, (size_t)need);
    if (rc) return rc;
    e->gather_cap = need;
  }
  hipLaunchKernelGGL(pack_gather_slot, dim3(1), dim3(256), 0, e->st, e->d_norm.get(), e->d_info.get(), e->d_fail.get(), e->d_iscal.get(), ns,
                     slot_sites, e->d_gather.get());
  HIPCHK(e, hipGetLastError());
  *d_slot = e->d_gather.get();
  *st = e->st;
  if (n_sites) *n_sites = ns;
  return PGBP_OK;
}
// the records of the listed beliefs of one site <-> a device buffer of the CALLER (pgbp_comm's send slot / a rank's part of
// its receive buffer), on the engine's stream: the device halves of pgbp_pack_beliefs / pgbp_unpack_beliefs
int engine_pack_records_device(pgbp_engine* e, int32_t site, int32_t n, const int32_t* beliefs, double* d_buf, int to_buf,
                               hipStream_t* st, int64_t* total) {
  if (!e || n < 0 || (n > 0 && (!beliefs || !d_buf))) return PGBP_ERR_INVALID;
  DeviceScope device_scope(e);
  int64_t tot = 0;
  int rc = xbuf_prepare(e, site, n, beliefs, &tot);
  if (rc) return rc;
  if (n > 0) {
    if (!to_buf) e->sym_known = false;
    launch_pack_records(e->d_pool.get() + (int64_t)site * e->plan.pool_stride(), e->d_xoff.get(), e->d_xoff.get() + n, n, d_buf, to_buf, e->st);
    HIPCHK(e, hipGetLastError());
  }
  if (st) *st = e->st;
  if (total) *total = tot;
  return PGBP_OK;
}
int engine_fail(pgbp_engine* e, int code, const std::string& msg) { return e->fail(code, msg); }
int engine_device(const pgbp_engine* e) { return e->plan.device; }
int engine_n_sites(const pgbp_engine* e) { return e->plan.n_sites; }
// pgbp_moments.hip: the belief state in the plain site-major layout (a univariate batch leaves its site-minor buffers first)
int engine_view(pgbp_engine* e, EngineView* v) {
  DeviceScope device_scope(e);
  if (e->layout_sm) {
    const int rc = ensure_site_minor(e, false);
    if (rc) return rc;
  }
  *v = engine_peek(e);
  return PGBP_OK;
}
EngineView engine_peek(pgbp_engine* e) {
  EngineView v;
  v.plan = &e->plan;
  v.st = e->st;
  v.pool = e->d_pool.get();
  v.boff = e->d_boff.get();
  v.bdim = e->d_bdim.get();
  v.bs16 = e->layout_bs16 ? 1 : 0;
  return v;
}
UniView engine_uni_view(pgbp_engine* e) {
  UniView u;
  u.tps = uni_engine(e) ? 1 : 0;
  u.sm = e->layout_sm ? 1 : 0;
  u.bs16 = e->layout_bs16 ? 1 : 0;
  u.pool = e->layout_sm ? e->sm.pool.get() : e->d_pool.get();
  u.stride = e->layout_sm ? sm_row(e->plan.n_sites) : e->plan.pool_stride();
  u.off = e->layout_sm ? e->d_packed_off.get() : e->d_boff.get();
  u.bdim = e->d_bdim.get();
  return u;
}
const Plan* engine_plan(const pgbp_engine* e) { return &e->plan; }
const LgModel* engine_lg(const pgbp_engine* e) { return e->lg.get(); }
}  // namespace pgbp
