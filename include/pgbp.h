/*
 * pgbp.h -- C ABI of the MI355X-native Gaussian belief-propagation calibration engine.
 *
 * Drop-in boundary for the message-passing hot path of
 * JuliaPhylo/PhyloGaussianBeliefProp.jl (reference paths relative to its repo root).
 * The reference has no FFI of its own; each entry point below replaces one Julia
 * function (cited), and is what a Julia `@ccall` shim binds.
 *
 * Conventions
 *   - all indices 0-based (the shim converts from Julia's 1-based);
 *   - a "belief" is a cluster (index < n_clusters) or a sepset (index >= n_clusters),
 *     clusters first, exactly like ClusterGraphBelief.belief (src/clustergraphbeliefs.jl:26-53);
 *   - "packed" belief storage = for each belief in index order: J (m*m doubles,
 *     column-major, full square), h (m), g (1); no padding; `pgbp_packed_size` doubles
 *     per site.  This is byte-for-byte what Julia's Matrix{Float64}/Vector{Float64}
 *     hold (src/beliefs.jl:122-127);
 *   - a directed message id is 2*k + dir for sepset k = (a, b): dir 0 is the message
 *     RECEIVED by a (sent by b), dir 1 the message received by b -- the (receiver, sender)
 *     key convention of ClusterGraphBelief.messageresidual (src/clustergraphbeliefs.jl:11-20);
 *   - n_sites >= 1 independent replicas ("sites": same graph, same scopes, different
 *     numbers) live in one engine; packed buffers are site-major;
 *   - every function returns PGBP_OK (0) or an error code; text via pgbp_last_error;
 *   - an engine owns one HIP stream; calls on one engine are not re-entrant
 *     (same as the reference: src/calibration.jl has no locking).
 *   - there is NO CPU fallback: pgbp_create fails with PGBP_ERR_NO_DEVICE without a GPU.
 */
#ifndef PGBP_H
#define PGBP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PGBP_VERSION 1
#define PGBP_MAX_DIM 384 /* largest belief dimension the kernels accept (refused above).  Up to 128 variables the working
                            matrix of a message ([J | h]: 128 x 129 doubles = 132 KB) lives in a CU's 160 KB of LDS; above,
                            in a workspace in global memory that stays in the L2 (the 54-node clique of the reference's
                            documented clique tree, docs/src/man/clustergraphs.md:40-89, has 162 / 216 / 324 variables with
                            3 / 4 / 6 traits).  The scores and the KL residuals have the same two paths: in LDS up to 96
                            (residual_kldiv!: two systems side by side; free_energy) variables, in the workspace
                            above -- no size of the reference's is refused below PGBP_MAX_DIM (src/beliefs.jl:1060-1075 and
                            src/score.jl:162-182 have no bound). */

enum pgbp_status {
  PGBP_OK = 0,
  PGBP_ERR_INVALID = 1,    /* malformed description / argument (ErrorException in the reference: src/beliefs.jl:398-401) */
  PGBP_ERR_HIP = 2,        /* HIP runtime error */
  PGBP_ERR_NOT_TREE = 3,   /* a schedule entry is not a preorder edge list of a tree (src/clustergraph.jl:885-894) */
  PGBP_ERR_TOO_LARGE = 4,  /* a belief dimension exceeds PGBP_MAX_DIM, or more than 65535 sites of dimension > 2 */
  PGBP_ERR_NO_DEVICE = 5,  /* no HIP device: the engine has no CPU path */
  PGBP_ERR_STATE = 6       /* call out of order (e.g. calibrate before set_schedule) */
};

/* Static description of a cluster graph with allocated scopes: what
 * allocatebeliefs (src/beliefs.jl:478-594) + ClusterGraphBelief (src/clustergraphbeliefs.jl:89-109)
 * establish, with scopeindex(sepset, cluster) (src/beliefs.jl:389-405) precomputed once. */
typedef struct pgbp_desc {
  int32_t n_clusters;
  int32_t n_sepsets;
  const int32_t* dims;            /* [n_clusters + n_sepsets] dimension(belief) */
  const int32_t* sepset_clusters; /* [2*n_sepsets] the two incident clusters (a, b) of each sepset */
  const int64_t* scope_off;       /* [2*n_sepsets + 1] offsets into scope_idx; entry 2k+side */
  const int32_t* scope_idx;       /* scopeindex(sepset k, cluster a) then (sepset k, cluster b): positions
                                     of the sepset's variables inside the cluster, strictly increasing */
  int32_t n_sites;                /* >= 1 */
  int32_t device;                 /* HIP device ordinal */
} pgbp_desc;

/* calibrate! keyword arguments (src/calibration.jl:35-44) and the tolerance of
 * iscalibrated_residnorm! (src/beliefs.jl:994). */
typedef struct pgbp_opts {
  int32_t auto_stop;           /* auto */
  int32_t update_residualnorm; /* default 1 */
  int32_t update_residualkldiv;/* default 0 (src/calibration.jl:43); 1: residual_kldiv! after every message */
  int32_t reserved;
  double  atol;                /* 1e-5 */
} pgbp_opts;

/* Outcome of a traversal / calibration for one site. */
typedef struct pgbp_result {
  int32_t succ;         /* 1 unless a message failed (first tuple element of calibrate!: src/calibration.jl:59,82) */
  int32_t iscal;        /* iscalibrated_residnorm(beliefs) (src/clustergraphbeliefs.jl:168-169) */
  int32_t iter_reached; /* 1-based iteration / schedule tree at which calibration was first reached   */
  int32_t tree_reached; /*   ("calibration reached: iteration $i, schedule tree $j", src/calibration.jl:54); 0 if never */
  int32_t fail_iter;    /* 1-based iteration / tree / direction (0 post, 1 pre) / edge (0-based position in  */
  int32_t fail_tree;    /*   the tree's edge list) of the FIRST failing message in the reference's sequential */
  int32_t fail_dir;     /*   order (src/calibration.jl:121,147); fail_info = PosDefException.info             */
  int32_t fail_edge;    /*   (src/beliefupdates.jl:69-76). All 0 / -1 when succ == 1.                          */
  int32_t fail_info;
  int32_t reserved;
} pgbp_result;

typedef struct pgbp_engine pgbp_engine; /* opaque: device-resident ClusterGraphBelief */
typedef struct pgbp_plan pgbp_plan;     /* opaque: host-only layout + level schedule (no GPU needed) */

/* ---- host-only planning (no GPU): layout, message table, level schedule ------------- */
/* On failure *out still receives a plan object that only carries the message for pgbp_plan_last_error; destroy it. */
int  pgbp_plan_create(const pgbp_desc* desc, pgbp_plan** out);
void pgbp_plan_destroy(pgbp_plan* p);
/* schedule = vector of spanning trees, each the (pa_j, ch_j) index vectors of
 * spanningtree_clusterlist in preorder (src/clustergraph.jl:885-894); tree t owns
 * entries [tree_off[t], tree_off[t+1]). */
int  pgbp_plan_set_schedule(pgbp_plan* p, int32_t n_trees, const int32_t* tree_off,
                            const int32_t* pa_j, const int32_t* ch_j);
int64_t pgbp_plan_packed_size(const pgbp_plan* p);    /* doubles per site, beliefs */
int64_t pgbp_plan_residual_size(const pgbp_plan* p);  /* doubles per site, residuals: per message dJ (s*s) then dh (s) */
int32_t pgbp_plan_n_messages(const pgbp_plan* p);     /* 2 * n_sepsets */
/* level structure of one traversal (dir 0 = postorder, 1 = preorder): number of levels,
 * tasks and message entries; then the arrays (caller-allocated):
 * level_off[n_levels+1] -> tasks, task_off[n_tasks+1] -> entries,
 * entry_msg[n_entries] directed message id, entry_edge[n_entries] position in the tree's edge list,
 * entry_reuse[n_entries] 1 if the marginal of the previous entry of the task is reused; 2: the entry is the PROLOGUE of
 * the next entry of its task (pgbp_plan_prologues). */
int  pgbp_plan_traversal_sizes(const pgbp_plan* p, int32_t tree, int32_t dir,
                               int32_t* n_levels, int32_t* n_tasks, int32_t* n_entries);
int  pgbp_plan_traversal(const pgbp_plan* p, int32_t tree, int32_t dir, int32_t* level_off,
                         int32_t* task_off, int32_t* entry_msg, int32_t* entry_edge, int32_t* entry_reuse);
/* level_nfast[n_levels]: how many tasks of each level (they come first) run on the register-resident
 * kernel; the rest run on the generic in-LDS kernel. */
int  pgbp_plan_level_nfast(const pgbp_plan* p, int32_t tree, int32_t dir, int32_t* level_nfast);
/* Launch form of the fast-class tasks of one traversal (caller-allocated arrays, any may be NULL):
 * level_ngroups[n_levels]: workgroup passes ("groups" of 4 wavefront records) of each level;
 * *tail_levels: how many levels at the root end of the schedule tree (the last ones of a postorder, the first of a
 *   preorder) are walked by the single-workgroup tail launch (8 records per level);
 * records[6 * 4 * sum(level_ngroups)], tail_records[6 * 8 * tail_levels]: per record {valid, message id, first record of
 *   its task inside the group, records of the task, record that computes its marginal, mode bits (1 own receiver
 *   block, 2 accumulate task, 4 the accumulate task only touches the receiver's g, 8 the record has a prologue:
 *   pgbp_plan_prologues)}. */
int  pgbp_plan_groups(const pgbp_plan* p, int32_t tree, int32_t dir, int32_t* level_ngroups, int32_t* tail_levels,
                      int32_t* records, int32_t* tail_records);
/* Chunks of fused levels of one traversal: runs of narrow levels below the tail that go out as ONE launch each, one
 * workgroup per dependency-closed tree of tasks, a workgroup barrier between its levels.  *n_chunks; then (any may be
 * NULL) info[4 * n_chunks] = {first level, one past the last level, workgroups, groups} per chunk (groups < 0: a chunk
 * of generic-class tasks, |groups| groups of 8 TASK ids); wg_off[sum(workgroups + 1)]: per chunk, the group range of each of
 * its workgroups (relative to the chunk's first group); records[6 * 8 * sum(|groups|)]: chunk after chunk, 8 records per
 * group -- as for pgbp_plan_groups, or {1, task index in pgbp_plan_traversal's task_off, 0, 0, 0, 0} / all 0 for a generic
 * chunk. */
int  pgbp_plan_chunks(const pgbp_plan* p, int32_t tree, int32_t dir, int32_t* n_chunks, int32_t* info, int32_t* wg_off,
                      int32_t* records);
/* PROLOGUES of the records above (any may be NULL): one word per record of pgbp_plan_groups' records / tail_records and
 * of pgbp_plan_chunks' records, in the same order: the directed message X -> F the record's wavefront sends first -- F the
 * sender of the record's own message, the message lands on the block that one integrates out and integrates nothing
 * itself (a variable cluster of a Bethe graph into a factor cluster) -- or -1.  In pgbp_plan_traversal such a message is
 * the entry in front of the record's own, in the same task. */
int  pgbp_plan_prologues(const pgbp_plan* p, int32_t tree, int32_t dir, int32_t* level_pro, int32_t* tail_pro,
                         int32_t* chunk_pro);
/* LEAF SEPSETS (any may be NULL): one word per record, order as for pgbp_plan_prologues: 1 where the record is a preorder
 * message into a leaf L of the schedule tree whose postorder message on the same edge is L's whole belief (nothing
 * integrated, sepset dimension = cluster dimension).  In a postorder + preorder pair the sepset then holds exactly what L
 * holds, and the register-resident kernels take it from L's block instead of loading it (PGBP_TUNING leaf_sepset=0: they
 * load it). */
int  pgbp_plan_leaf_sepset(const pgbp_plan* p, int32_t tree, int32_t dir, int32_t* level_leaf, int32_t* tail_leaf,
                           int32_t* chunk_leaf);
/* CHAINS of the loop launches in the packed layout (csrc/pgbp_loop.hip), one word per record of the tail and of the chunks
 * (order as above; either may be NULL): kind | source record of the previous group << 8 | late << 16.  A workgroup loads
 * the operands of a group while the group before it still runs: kind 1 / 3 = the integrated block of the record's 2P-dim
 * sender / its P-dim sender's whole belief, 2 = the X of its prologue, was stored by that source record in the group
 * before and reaches this one through the workgroup's LDS; late = the group reads from memory something else the group
 * before it writes, or is the first of its walk: the workgroup waits for every store and loads at the group's top. */
int  pgbp_plan_chains(const pgbp_plan* p, int32_t tree, int32_t dir, int32_t* tail_chain, int32_t* chunk_chain);
/* The self-contained message records of the wave-per-task kernels (one 128-byte record per message of a generic-class
 * task; layout: struct GRec in csrc/pgbp_internal.hpp -- offsets of sender / receiver / sepset / residual inside a
 * site's pools, message id, sequence number, beliefs, index-pool offsets of the three maps, `next` = the record of the
 * task's next message or -1, dimensions {mf, mt, s, ni}, first kept / updated index when contiguous (255: not), reuse
 * flag, inline bits, perm[40] = the sender's variables, integrated first, kept last (bit 0), up[16] = the receiver's
 * positions (bit 1)).  *n_records; then (any may be NULL) level_first[n_levels] = the record of the level's first
 * generic-class task (its tasks follow in task order), task_first[n_tasks] = the first record of every task (-1: a
 * fast-class task), records[128 * n_records]. */
int  pgbp_plan_records(const pgbp_plan* p, int32_t tree, int32_t dir, int32_t* n_records, int32_t* level_first,
                       int32_t* task_first, uint8_t* records);
/* The ROW form of the postorder levels whose generic-class tasks are all small (at most 8 integrated and 8 kept variables)
 * and have at most four messages into their receiver: the level's messages one per row of 16 lanes (four rows = one
 * wavefront of bp_level_small4), the rows of a task consecutive, in the task's order, inside one wavefront.  *n_rows over
 * the traversal; then (any may be NULL) level_row0[n_levels], level_nrows[n_levels] (a multiple of four; 0: the level has
 * no row form) and rowmap[2 * n_rows] = pairs {record of pgbp_plan_records or -1 (an empty row), position in the task |
 * messages of the task << 8}.  mult! into a receiver happens in the order of the positions: the sequential task's sums. */
int  pgbp_plan_rows(const pgbp_plan* p, int32_t tree, int32_t dir, int64_t* n_rows, int64_t* level_row0,
                    int32_t* level_nrows, int32_t* rowmap);
/* The LEVELLED walk of regularizebeliefs_onschedule! (src/clustergraphbeliefs.jl:376-403; pgbp_regularize_onschedule),
 * built on first use.  The walk visits the clusters in index order; every sepset carries one message, from its lower
 * cluster to its higher one, sent in the walk's order (clusters, then each one's sepsets in index order).
 * cluster_level[n_clusters]: level of the cluster's step (its eps edits) = 1 + the largest level of a message into it (0: none);
 * msg_level[2*n_sepsets]: level of each directed message, -1 unsent: max(cluster_level[sender], level of the previous
 * message into the same receiver), so that the messages into a receiver keep the walk's order;
 * walk_pos[2*n_sepsets]: position of each sent message in the walk's order, -1 unsent.  Any pointer may be NULL. */
int  pgbp_plan_onschedule(const pgbp_plan* p, int32_t* n_levels, int32_t* cluster_level, int32_t* msg_level,
                          int32_t* walk_pos);
const char* pgbp_plan_last_error(const pgbp_plan* p);

/* ---- engine lifetime ------------------------------------------------------------------ */
/* ClusterGraphBelief(beliefs, ...) constructor (src/clustergraphbeliefs.jl:89-109): allocates
 * beliefs, factors, message residuals (flags false / kldiv -1; empty messages born calibrated:
 * src/beliefs.jl:914-924) on the device. */
int  pgbp_create(const pgbp_desc* desc, pgbp_engine** out);
void pgbp_destroy(pgbp_engine* e);
const char* pgbp_last_error(const pgbp_engine* e); /* e == NULL: error of the last failed create */
int64_t pgbp_packed_size(const pgbp_engine* e);
int64_t pgbp_residual_size(const pgbp_engine* e);
int32_t pgbp_n_messages(const pgbp_engine* e);
int32_t pgbp_belief_dim(const pgbp_engine* e, int32_t belief); /* dimension of a cluster / sepset belief, -1: bad index */

/* ---- state transfer ------------------------------------------------------------------- */
/* Upload all beliefs of all sites (packed, site-major; host pointer). If snapshot_factors != 0 the
 * cluster part is also stored as the factors (init_factors_allocate, src/beliefs.jl:628-637). */
int  pgbp_set_beliefs(pgbp_engine* e, const double* packed, int32_t snapshot_factors);
int  pgbp_get_beliefs(pgbp_engine* e, double* packed);
int  pgbp_set_belief(pgbp_engine* e, int32_t site, int32_t belief, const double* rec); /* J,h,g of one belief */
int  pgbp_get_belief(pgbp_engine* e, int32_t site, int32_t belief, double* rec);
/* The EXCHANGE BUFFER of a cluster graph cut across devices (the roots of the subtrees a rank owns
 * before the top of a traversal, the records it owns after one): the records (J, h, g; the plain packing of
 * pgbp_get_belief) of `n` listed beliefs of one site, back to back in the order of the list -- gathered on the device
 * into one contiguous buffer and moved across the bus once (pack), or the reverse (unpack: overwrites those beliefs).
 * pgbp_packed_beliefs_size: doubles in that buffer (-1: a bad index).  This is the calibration loop's only exchange
 * when the traversals of src/calibration.jl:111-161 are cut by spanning-tree subtrees (sharding.py: NetworkCut). */
int64_t pgbp_packed_beliefs_size(pgbp_engine* e, int32_t n, const int32_t* beliefs);
int  pgbp_pack_beliefs(pgbp_engine* e, int32_t site, int32_t n, const int32_t* beliefs, double* buf);
int  pgbp_unpack_beliefs(pgbp_engine* e, int32_t site, int32_t n, const int32_t* beliefs, const double* buf);
/* all beliefs of ONE site (packed: pgbp_packed_size doubles): what a host reads back into the arrays of one
 * ClusterGraphBelief of a batch without downloading the other sites */
int  pgbp_get_site_beliefs(pgbp_engine* e, int32_t site, double* packed);
/* init_factors_frombeliefs! (src/beliefs.jl:746-761) */
int  pgbp_init_factors_frombeliefs(pgbp_engine* e);
/* init_beliefs_reset_fromfactors! (src/clustergraphbeliefs.jl:126-139) */
int  pgbp_reset_from_factors(pgbp_engine* e);
/* init_messagecalibrationflags_reset!(beliefs, reset_kl) (src/clustergraphbeliefs.jl:146-150) */
int  pgbp_reset_flags(pgbp_engine* e, int32_t reset_kl);
/* MessageResidual fields of every directed message, site-major: dJ,dh packed (pgbp_residual_size
 * doubles per site), iscalibrated_resid flags, kldiv and iscalibrated_kl flags (n_messages per site).
 * Any pointer may be NULL. */
int  pgbp_get_residuals(pgbp_engine* e, double* packed, int32_t* iscalibrated_resid, double* kldiv,
                        int32_t* iscalibrated_kl);
/* The same for ONE directed message of one site -- message 2k + dir is the one RECEIVED by end `dir` of sepset k
 * (messageresidual[(receiver, sender)], src/clustergraphbeliefs.jl:17-20): rec = dJ (s*s, column-major) then dh (s).
 * What a host that keeps the reference's objects fetches on first access after a calibrate! instead of downloading
 * every residual (the lazy write-back of INTEGRATION.md).  Any of the four output pointers may be NULL. */
int  pgbp_get_residual(pgbp_engine* e, int32_t site, int32_t msg, double* rec, int32_t* iscalibrated_resid, double* kldiv,
                       int32_t* iscalibrated_kl);

/* ---- the hot path ------------------------------------------------------------------------ */
int  pgbp_set_schedule(pgbp_engine* e, int32_t n_trees, const int32_t* tree_off,
                       const int32_t* pa_j, const int32_t* ch_j);
/* propagate_belief!(cluster_to, sepset, cluster_from, residual) (src/beliefupdates.jl:634-665) for
 * every site. info[site] = 0 ok, > 0 PosDefException.info (belief state of that site untouched,
 * exception "returned not thrown"); `sepset` is a belief index (>= n_clusters). */
int  pgbp_propagate(pgbp_engine* e, int32_t cluster_to, int32_t sepset, int32_t cluster_from,
                    const pgbp_opts* opts, int32_t* info);
/* residual_kldiv!(messageresidual[(to, from)], sepset) (src/beliefs.jl:1060-1075) for every site, for the
 * message last sent from cluster_from to cluster_to: updates that residual's kldiv and iscalibrated_kl
 * (left alone if the sepset belief, or the one before the message, is not positive definite).
 * iscalibrated_kl[n_sites] (may be NULL) receives the flag. */
int  pgbp_residual_kldiv(pgbp_engine* e, int32_t cluster_to, int32_t sepset, int32_t cluster_from,
                         const pgbp_opts* opts, int32_t* iscalibrated_kl);
/* regularizebeliefs_bycluster!(beliefs, clustergraph) (src/clustergraphbeliefs.jl:235-275) on the device:
 * per cluster eps = max(eps(Float64), max|J|); +eps on the cluster's diagonal at the scope of each
 * incident sepset, and on the sepset's diagonal.  Asynchronous on the engine's stream. */
int  pgbp_regularize_bycluster(pgbp_engine* e);
/* regularizebeliefs_onschedule!(beliefs, clustergraph) (src/clustergraphbeliefs.jl:343-403) on the device, for the sites
 * [site_begin, site_end) (other sites untouched): clusters in index order, each adds eps = max(max|J|, sqrt(eps(Float64)))
 * on its diagonal at the scope of every sepset to a later neighbour and on that sepset's diagonal, then sends its real
 * message (propagate_belief!, as pgbp_propagate: same arithmetic, bit for bit) to those neighbours in sepset order --
 * level by level (pgbp_plan_onschedule), a few launches per level, one synchronisation at the end.
 * fail_msg[n_sites] = directed message id of the first failing message in walk order or -1, fail_info[n_sites] =
 * PosDefException.info or 0 (either may be NULL; sites outside the range get -1 / 0).  A failed site is left with every
 * message before the failure in walk order applied; the failed message leaves its receiver, sepset and residual as
 * pgbp_propagate does; messages later in walk order that do not depend on the failure, and the eps edits of later
 * clusters, may already be applied. */
int  pgbp_regularize_onschedule(pgbp_engine* e, int32_t site_begin, int32_t site_end, const pgbp_opts* opts,
                                int32_t* fail_msg, int32_t* fail_info);
/* propagate_1traversal_postorder! / _preorder! (src/calibration.jl:111-161), dir 0 / 1.
 * results[n_sites]: succ, fail_* filled. */
int  pgbp_traverse(pgbp_engine* e, int32_t tree, int32_t dir, const pgbp_opts* opts, pgbp_result* results);
/* calibrate!(beliefs, schedule, niter; ...) (src/calibration.jl:35-84). results[n_sites].
 * With auto_stop EVERY SITE stops at the first schedule tree at which that site is calibrated, exactly the reference's
 * `auto` run on that site alone (the device skips the site's later traversals; results[s].iter_reached / tree_reached say
 * where it stopped); the call returns when every site has reached calibration or failed, or after niter iterations. */
int  pgbp_calibrate(pgbp_engine* e, int32_t niter, const pgbp_opts* opts, pgbp_result* results);
/* integratebelief!(obj, beliefindex) (src/clustergraphbeliefs.jl:194, src/beliefupdates.jl:168-200) for
 * every site: mu[n_sites * m] (may be NULL), norm[n_sites], info[n_sites] (0 ok, >0 not PD, may be NULL).
 * An all-zero belief gives mu = Inf, norm = g (src/beliefupdates.jl:189-191). */
int  pgbp_integrate(pgbp_engine* e, int32_t belief, double* mu, double* norm, int32_t* info);
/* integratebelief! (src/beliefupdates.jl:168-200) for MANY beliefs at once, with the covariance: one launch per dimension
 * class over a grid of (belief, site) -- at most 16 variables: four beliefs per wavefront, one per row of 16 lanes, in
 * registers; 17 .. 64: one wavefront per belief, the working matrix in LDS; 65 .. 128: a workgroup of 256 threads, the
 * working matrix in up to 133 KB of LDS, the inverse formed in place from the elimination's factor (csrc/pgbp_moments.hip).
 * beliefs[n]: belief indices (NULL: all clusters, n ignored); sites [site_begin, site_end).
 * Per (site, listed belief) of dimension m, back to back in list order, site-major:
 *   out    : Sigma = J^-1 (m*m, column-major, symmetric, both triangles written), then mu (m), then norm (1)
 *            -- the layout of a belief record (pgbp_get_belief), so pgbp_packed_beliefs_size gives the size;
 *   with want_cov == 0 only mu (m) then norm (1) are written.
 * info[(site - site_begin) * n + i] (may be NULL): 0, or the PosDefException.info of that belief (its outputs are NaN).
 * An all-zero belief gives mu = Inf, norm = g (src/beliefupdates.jl:189-191), info 0; the reference defines no
 * covariance there, so Sigma is all NaN.  A belief of dimension 0 gives norm = g.
 * mu and norm are bit-identical to pgbp_integrate's in every class (the same operations on every entry, in the same
 * order), on the plain and on the packed (BS16) layout.  A univariate batch in the site-minor layout is first converted
 * to the plain one (as pgbp_free_energy does); pgbp_integrate has a closed form of its own there (dimension <= 2), so
 * on such an engine the two agree to rounding (1e-12 relative), not bit for bit.
 * A listed belief of more than 128 variables, or an index out of range, fails with PGBP_ERR_INVALID (the message names
 * the belief) before anything is launched.  Read-only on the beliefs; no atomics: a second call returns the same bytes.
 * The outputs and the info words come back as two copies behind one stream synchronisation (the call's scratch buffers are
 * allocated and freed per call, which synchronises the device as well).
 * pgbp_moments_size: doubles per site of `out` (-1: a bad list). */
int pgbp_moments(pgbp_engine* e, int32_t n, const int32_t* beliefs, int32_t site_begin, int32_t site_end,
                 int32_t want_cov, double* out, int32_t* info);
int64_t pgbp_moments_size(pgbp_engine* e, int32_t n, const int32_t* beliefs, int32_t want_cov);
/* The loop of calibrate_exact_cliquetree! (src/calibration.jl:442-499) over the families given to pgbp_lg_setup, on the
 * CURRENT beliefs (calibrated under R = I and an improper root prior), for sites [site_begin, site_end):
 * num[(site - site_begin) * p*p ...] (column-major p x p) and den[site - site_begin]; R_hat = num / den.
 * One workgroup per (family, site) computes the moments of the family's cluster in LDS (the solve of pgbp_moments; only the
 * family's diffExp, t = sum gamma^2 length and 1 - diffVar / t leave it, into a per-family slot), a second pass adds the
 * slots in family order by a fixed tree: no atomics on doubles, the same bytes on every call.  Line by line the reference:
 * a family with t == 0, a root-prior family, a tip whose parent (an internal child that itself) has nothing in scope and a
 * tip without data are skipped; a tip's denominator term reads the cluster's FIRST variable (vv[1, 1], :478), which must
 * be its parent's first trait (checked); an internal family reads J^-1 at the first trait of the child and of each parent.
 * Fails before any launch with PGBP_ERR_STATE without a family table, with PGBP_ERR_INVALID for a family whose parent is
 * the fixed root (the sweep is defined on the improper-root engine), for partial scopes ("some leaf must have partial
 * data: cluster ... has partial traits in scope", :416-421) and for a cluster of more than 128 variables.
 * info[site - site_begin] (may be NULL) as pgbp_free_energy: 0, or 1-based index of the first cluster that is not positive
 * definite (num and den of that site are NaN). */
int pgbp_bm_exact_stats(pgbp_engine* e, int32_t site_begin, int32_t site_end, double* num, double* den, int32_t* info);
/* The exact gradient of the log-likelihood with respect to every model parameter, from the CURRENT beliefs, for sites
 * [site_begin, site_end): Fisher's identity d loglik / d theta = sum_f E[d log phi_f / d theta | data] over the families
 * given to pgbp_lg_setup, the expectation under the belief of the family's cluster, with the parameters the engine kept from
 * the last pgbp_lg_assignfactors (shared or per site: a per-site engine returns each site's own gradient).
 * THE RESULT IS THE EXACT GRADIENT ONLY WHEN THE BELIEFS ARE CALIBRATED (postorder AND preorder) ON A CLIQUE TREE UNDER THE
 * PARAMETERS OF THE LAST pgbp_lg_assignfactors; the call does not verify that.  On a loopy cluster graph the same sweep on
 * the beliefs of a CONVERGED calibration is the gradient of the factored energy (the Bethe free energy is stationary in the
 * beliefs at a fixed point); before convergence it is neither.
 * Per family (notation of pgbp_lg_params: residual r = x_child - sum_k qc_k x_k - w, variance V = sum_k vc_k R[colour_k]
 * restricted to the kept components O = child_mask, j = V_OO^-1; blocks in scope random with the cluster's J^-1 h and J^-1,
 * a tip's data row and the fixed root's mean constants): e = E[r], M = Cov(r) + e e', G_V = (j M j - j) / 2, g_w = j e,
 * g_qk = E[r' j x_k].  Outputs, site-major:
 *   dR     [sites][n_rates][p*p] column-major, symmetric: dR[c] = sum_f sum_{k: colour_k = c} vc_k G_V(f) (a root-prior
 *          family: G_V itself), so that d loglik = tr(dR[c] dR_c): entry (a, b) is the derivative along (E_ab + E_ba) / 2;
 *   dmu    [sites][p]: j e of the root-prior family plus qc_k j e of the families whose parent k is the fixed root (zero
 *          for an improper root);
 *   dtheta [sites][p], dalpha [sites] (OU; NULL allowed for a BM engine, zeros are written when given there):
 *          dtheta = sum wc_k g_w,  dalpha = sum_k (dvc_k/dalpha tr(G_V R[colour_k]) + dwc_k/dalpha theta' g_w +
 *          dqc_k/dalpha g_qk), R the stationary variance.
 * Families the factor fill skips (child_mask == 0) contribute nothing.
 * Device (csrc/pgbp_grad.hip): one workgroup per (family, site) solves the family's cluster in LDS (the solve of
 * pgbp_moments) and writes a slot of p*p + p + 3 + n_rates doubles; the slots are added in a fixed order (256 consecutive
 * families per workgroup, then a fixed tree): no atomics on doubles, two calls return the same bytes.  The slots of a chunk
 * of sites at a time (256 MB at most).  Read-only on the beliefs; every layout (a site-minor univariate batch is converted
 * to the plain layout first, as pgbp_bm_exact_stats does).
 * Fails before any launch with PGBP_ERR_STATE without a family table or before the first pgbp_lg_assignfactors, with
 * PGBP_ERR_INVALID for a site range out of bounds, for dalpha / dtheta NULL on an OU engine, for a family whose cluster has
 * more than 128 variables, and when that cluster's working matrix plus the p x p scratch exceed the 160 KB of LDS (p > 16
 * with clusters near 128 variables).  Fixed, random and improper roots, hybrid families, several colours and scope masks
 * are all accepted.
 * info[site - site_begin] (may be NULL): 0, or the 1-based index of the first cluster that is not positive definite (or
 * whose family variance is not): that site's outputs are NaN. */
int pgbp_lg_gradient(pgbp_engine* e, int32_t site_begin, int32_t site_end, double* dR, double* dmu, double* dalpha,
                     double* dtheta, int32_t* info);
/* DERIVATIVES OF THE LOG-LIKELIHOOD IN EVERY EDGE -- its length, its inheritance and a shift of the mean on it -- from the
 * CURRENT beliefs and the parameters the engine kept from the last pgbp_lg_assignfactors (shared or per site), for sites
 * [site_begin, site_end).  The same Fisher's-identity sweep as pgbp_lg_gradient, without its sum over the families, and exact
 * under the same condition: beliefs calibrated (postorder AND preorder) on a clique tree under those parameters; not verified.
 * Per family f, with O = child_mask, j = V_OO^-1 and e, M, G_V = (j M j - j) / 2, g_w = j e, g_qk = E[r' j x_k] as documented
 * for pgbp_lg_gradient, per parent edge k < n_parents[f]:
 *     dX_k = dvc_k/dX tr(G_V R[colour_k]_OO) + dwc_k/dX theta_O' g_w + dqc_k/dX g_qk,     X in {length t, inheritance gamma},
 *     BM:                    d/dt: dqc = 0, dvc = gamma^2, dwc = 0;                      d/dgamma: dqc = 1, dvc = 2 gamma t, dwc = 0;
 *     OU, a = exp(-alpha t): d/dt: dqc = -gamma alpha a, dvc = 2 gamma^2 alpha a^2, dwc = gamma alpha a;
 *                            d/dgamma: dqc = a, dvc = 2 gamma (1 - a^2), dwc = 1 - a.
 * Outputs, site-major; any of the three may be NULL, not all three:
 *   dlength [sites][n_families][K], dgamma [sites][n_families][K] (K = max_parents): entry k in the per-parent order given to
 *       pgbp_lg_setup.  dgamma is the FREE partial in each gamma_k; that a hybrid's gamma sum to 1 is the caller's constraint:
 *       d/dgamma_major at gamma_minor = 1 - gamma_major is dgamma[major] - dgamma[minor].  Entries k >= n_parents[f] are NaN
 *       (no such edge), every entry of a root-prior family included.  A family the factor fill skips (child_mask == 0)
 *       writes 0 for its real edges.
 *   dshift [sites][n_families][p]: the derivative in an additive displacement s of the child's conditional mean
 *       (r = x_child - sum_k qc_k x_k - w - s), that is g_w embedded into the p traits, 0 outside O.  For a tree edge this is
 *       the score of a mean shift on that edge; for a root-prior family it is the family's dmu term.  Skipped families: 0.
 *   info [sites] (may be NULL): as pgbp_lg_gradient's; that site's outputs are all NaN, other sites are unaffected.
 * Device (csrc/pgbp_edge.hip): one workgroup per (family, site) -- 64 threads while every family's cluster has at most 64
 * variables, else 256 -- solves the cluster in LDS (the solve of pgbp_moments), forms the family quantities and writes its
 * own K + K + p outputs: no reduction, no atomics on doubles, every sum in a fixed index order.  What a (family, site)
 * writes depends on nothing else in the call; two calls return the same bytes.  Device copies of the outputs of a chunk of
 * sites at a time (256 MB at most), one stream synchronisation per call.  Read-only on the beliefs; every layout, as
 * pgbp_lg_gradient.
 * Fails before any launch with PGBP_ERR_STATE without a family table or before the first pgbp_lg_assignfactors, with
 * PGBP_ERR_INVALID for a site range out of bounds, for all three outputs NULL, for a family whose cluster has more than 128
 * variables (the message names the family and the cluster), and when the LDS need -- the largest cluster's working matrix
 * plus p x (2p + 1) + 3 p x p doubles of family scratch -- exceeds 160 KB. */
int pgbp_lg_edge_gradient(pgbp_engine* e, int32_t site_begin, int32_t site_end, double* dlength, double* dgamma,
                          double* dshift, int32_t* info);
/* Replace the lengths and / or the inheritances of the family table on the device without a new pgbp_lg_setup: length and
 * gamma are [n_families * max_parents] as in pgbp_lg_families, either may be NULL (left as it is).  The per-cluster records
 * the thread-per-site fill keeps are rewritten too.  The checks of pgbp_lg_setup apply (lengths of real edges positive and
 * finite, inheritances finite): PGBP_ERR_INVALID with NOTHING changed.  Data, masks and parameters are left alone; beliefs
 * and factors are not refilled: the next pgbp_lg_assignfactors or pgbp_enqueue_loglik_lg uses the new values.
 * PGBP_ERR_STATE without a family table.  Two small copies and one stream synchronisation. */
int pgbp_lg_set_edges(pgbp_engine* e, const double* length, const double* gamma);
/* MEAN SHIFTS ON EDGES: the reference's HeterogeneousShiftedBrownianMotion (src/evomodels/heterogeneousmodels.jl:152-179) and
 * the displacement its generic factor code carries through tree edges and hybrid nodes (src/evomodels/evomodels.jl:208-245,
 * :314-330).  A shift s_k (a p-vector) on parent edge k of family f makes the child's conditional mean
 *     sum_k gamma_k (a_k x_k + (1 - a_k) theta + s_k),   a_k = 1 for BM, exp(-alpha t_k) for OU:
 * in the notation of pgbp_lg_params the family's offset gains d = sum_k gamma_k s_k, the residual is
 * r = x_child - sum_k qc_k x_k - w - d.  The coefficient of a shift is gamma_k under both models.  Variances, J and qc, vc, wc
 * are untouched; the factor keeps the components O = child_mask[f] of d: a component of a shift outside O has no effect (not
 * an error).
 *   edge  [n_shifts]: edge[i] = f * max_parents + k, the index used by length and gamma of pgbp_lg_families; the list is sparse
 *         (the device keeps a dense int32 slot map [n_families * max_parents], -1 for none, and the values);
 *   value [n_shifts][p], or with per_site != 0 [n_sites][n_shifts][p] (allowed whether the parameters are shared or per site);
 *   n_shifts = 0 clears the shifts (edge and value may be NULL).  The call REPLACES the previous list, it does not add to it.
 * Takes effect as pgbp_lg_set_edges does: the next pgbp_lg_assignfactors or pgbp_enqueue_loglik_lg uses the shifts (every fill is
 * followed by a correction of h and g of the clusters that hold a shifted family, csrc/pgbp_shift.hip: nothing is launched
 * when none is set); beliefs and factors are not refilled by this call.  pgbp_lg_gradient, pgbp_lg_edge_gradient, pgbp_lg_loo and
 * pgbp_lg_impute read the CURRENT shifts, as they read the current parameters: call them on beliefs calibrated under both.
 * There dgamma[f][k] gains s_k,O' g_w; dshift keeps its meaning: the derivative in s_k is gamma_k * dshift[f].  pgbp_moments and
 * pgbp_sample_posterior read beliefs only.  Shifts survive pgbp_lg_set_edges (gamma is read when the factors are filled); a new
 * pgbp_lg_setup clears them.  An engine borrowed from a pgbp_group or pgbp_patterns (pgbp_group_engine, pgbp_patterns_engine)
 * takes the call like any other; there is no group-level call.
 * PGBP_ERR_STATE without a family table.  PGBP_ERR_INVALID with NOTHING changed (the previous shifts stay in force) and a text
 * that names the entry for: an index out of range, k >= n_parents[f], a root-prior family (it has no edge), an edge listed
 * twice, a value that is not finite.  Up to four copies (the slot map, the cluster list, the values -- n_sites * n_shifts * p
 * doubles with per_site -- and, for a univariate per-site batch, their [shift][site] copy) and one stream synchronisation.
 * pgbp_lg_shift_count: the number of shifts in force (0: none; -1: no family table). */
int pgbp_lg_set_shifts(pgbp_engine* e, int32_t n_shifts, const int32_t* edge, const double* value, int32_t per_site);
int32_t pgbp_lg_shift_count(pgbp_engine* e);
/* PAINTED OPTIMA under PGBP_LG_OU (Hansen's model): theta painted on the edges as `color` paints the rates.  In the notation of
 * pgbp_lg_params the offset of family f is w = sum_k wc_k theta_{r(f,k)} instead of sum_k wc_k theta: w gains
 * d_opt = sum_k wc_k (theta_{r(f,k)} - theta) on the kept traits O = child_mask[f].  Variances, J, qc and vc are untouched.
 *   regime [n_families * max_parents] int32, indexed f * max_parents + k as length and gamma: 0 = the edge keeps theta of
 *          pgbp_lg_params, r in 1 .. n_regimes = its optimum is value[r - 1]; entries of a root-prior family and of
 *          k >= n_parents[f] are ignored;
 *   value  [n_regimes][p], or with per_site != 0 [n_sites][n_regimes][p] (allowed whether the parameters are shared or per site);
 *   n_regimes = 0 clears (regime and value may be NULL).  The call REPLACES the previous setting.
 * Takes effect as pgbp_lg_set_shifts does, at the next fill: the fill kernels keep their code and the optimum enters as a
 * displacement through the correction that follows every fill (csrc/pgbp_shift.hip: delta = the shifts' d + d_opt, the clusters
 * visited are those of either list); the tip-noise and the per-site-mask corrections form the same offset.  Under PGBP_LG_BM
 * wc = 0: the optima have no effect, nothing is launched for them and every byte is that of an engine without optima.
 * ACCURACY: "fill with theta, then add wc (theta_r - theta)" leaves an error of about 2^-52 |wc| (|theta| + |theta_r|) in w where
 * a direct fill would leave 2^-52 |wc theta_r|: nothing is lost while theta is of the size of the optima.
 * The optima survive pgbp_lg_set_edges, pgbp_lg_set_shifts, pgbp_lg_set_tip_noise and pgbp_lg_set_site_missing; a new
 * pgbp_lg_setup clears them.  An engine borrowed from a pgbp_group or pgbp_patterns takes the call like any other.
 * THE SWEEPS while optima are in force under PGBP_LG_OU: pgbp_moments, pgbp_sample_posterior, pgbp_posterior_cov and their
 * _sites twins read beliefs only and are unaffected.  pgbp_lg_gradient_optima and pgbp_lg_gradient_sites_optima (below) honour
 * them and return the derivative in every optimum.  pgbp_lg_gradient(_noise) and pgbp_lg_gradient_sites cannot return it -- and
 * their dtheta and dalpha would read as the unpainted model's --, and pgbp_lg_edge_gradient, pgbp_lg_shift_scan, pgbp_lg_loo,
 * pgbp_lg_impute, their _sites twins and pgbp_lg_simulate form w themselves and do not know the optima yet: each of these
 * REFUSES before any launch (PGBP_ERR_INVALID, naming the optima) with its outputs, the layout, the pool and the setting
 * untouched; none returns the unpainted answer.  Under PGBP_LG_BM they all run as without optima.
 * PGBP_ERR_STATE without a family table.  PGBP_ERR_INVALID with NOTHING changed (the previous optima stay in force) and a text
 * that names the entry for: a regime outside 0 .. n_regimes on a real edge, a value that is not finite.  Up to four copies (the
 * regime map, the cluster list, the values and, for a univariate per-site batch, their [regime][site] copy) and one stream
 * synchronisation.
 * pgbp_lg_optima_count: the number of regimes in force (0: none; -1: no family table). */
int pgbp_lg_set_optima(pgbp_engine* e, int32_t n_regimes, const int32_t* regime, const double* value, int32_t per_site);
int32_t pgbp_lg_optima_count(pgbp_engine* e);
/* The values of the setting in force alone -- what a fit moves at every step: `value` in the shape the setter was given
 * ([n_regimes][p], or [n_sites][n_regimes][p] when it was set per site) goes into the buffers the device already holds; the
 * regime map, the cluster list and the allocations stay (one or two copies, no allocation).  Takes effect at the next fill.
 * PGBP_ERR_STATE without a family table or without optima; PGBP_ERR_INVALID, with nothing changed, for a value that is not
 * finite. */
int pgbp_lg_update_optima(pgbp_engine* e, const double* value);
/* pgbp_lg_gradient_noise with one more output, doptima [sites][n_regimes][p] (n_regimes of pgbp_lg_optima_count; NULL only when
 * no optima are set; dsigma_e may be NULL).  With optima in force under PGBP_LG_OU:
 *   doptima[r] = sum over the edges (f, k) of regime r of wc_k g_w(f)   (a regime no edge carries: 0),
 *   dtheta     = the same sum over the edges of regime 0 only,
 *   dalpha     uses theta_{r(f,k)} in its dwc_k theta g_w term,
 * and dR, dmu, dsigma_e see the optima through e = E[r] only.  doptima is one more block of the family slot, added by the same
 * fixed tree as dR: two calls return the same bytes.  Without optima, and under PGBP_LG_BM, every other output holds the bytes
 * of pgbp_lg_gradient_noise and doptima holds zeros.
 * pgbp_lg_gradient_sites_optima: the same for pgbp_lg_gradient_sites (a univariate batch on the thread-per-site kernels),
 * doptima [sites][n_regimes].  The regime of an edge is uniform across a wavefront; a launch carries four regimes in registers
 * beside its four rates, more are swept in groups.  A site's bytes depend neither on the call nor on the site range or the
 * chunking.  The instance that runs without optima is the kernel of pgbp_lg_gradient_sites, unchanged. */
int pgbp_lg_gradient_optima(pgbp_engine* e, int32_t site_begin, int32_t site_end, double* dR, double* dmu, double* dalpha,
                            double* dtheta, double* dsigma_e, double* doptima, int32_t* info);
int pgbp_lg_gradient_sites_optima(pgbp_engine* e, int32_t site_begin, int32_t site_end, double* dR, double* dmu, double* dalpha,
                                  double* dtheta, double* dsigma_e, double* doptima, int32_t* info);
/* MEASUREMENT ERROR AT THE TIPS: species means with known standard errors, or means of n_f individuals with a within-species
 * covariance.  A tip family f (child_pos < 0, a data row, at least one parent edge) that is listed gets the conditional variance
 *     V_f = sum_k vc_k R[colour_k] + E_f,      E_f = scale_f * Sigma_e + diag(se2_f):
 * the tip's variable is the OBSERVATION y = x + eps, eps ~ N(0, E_f).  Means, qc, wc and the shifts are untouched; only the
 * observed block E_OO (O = child_mask[f]) enters the factor.
 *   family  [n]: the listed tip families; the list is sparse (the device keeps a dense int32 slot map [n_families], -1 for none);
 *   scale   [n]: scale_f >= 0, for example 1 / n_f;
 *   sigma_e [p][p] symmetric, diagonal >= 0 (the two triangles may differ by 1e-12 of the largest entry: they are averaged), or
 *           with per_site != 0 [n_sites][p][p];
 *   se2     NULL, or [n][p] known sampling variances >= 0, with per_site != 0 [n_sites][n][p];
 *   n = 0 clears the noise (the arrays may be NULL).  The call REPLACES the previous list, it does not add to it.
 * Takes effect as pgbp_lg_set_shifts does: the next pgbp_lg_assignfactors or pgbp_enqueue_loglik_lg uses it (every fill, and its
 * shift correction, is followed by a correction of J, h and g of the clusters that hold a noisy tip family,
 * csrc/pgbp_noise.hip: nothing is launched when none is set); beliefs and factors are not refilled by this call.  The sweeps
 * read the CURRENT noise as they read the current parameters and shifts: pgbp_lg_gradient(_noise), pgbp_lg_edge_gradient and
 * pgbp_lg_shift_scan use V_OO + E_OO for a noisy tip family; pgbp_lg_loo and pgbp_lg_impute then predict the OBSERVATION of a
 * noisy tip (variance V + E; pgbp_lg_impute uses the blocks E_PP, E_PO of the missing traits as well), not the trait value
 * under it.  The noise survives pgbp_lg_set_edges and pgbp_lg_set_shifts; a new pgbp_lg_setup clears it.  An engine borrowed
 * from a pgbp_group or pgbp_patterns takes the call like any other; there is no group-level call.
 * ACCURACY: the fill writes j = V_OO^-1 and the correction adds D = (V_OO + E_OO)^-1 - j, formed as -j E_OO (V_OO + E_OO)^-1:
 * the tip's contribution carries a relative error of about 2^-52 (1 + |E| / |V|).  At |E| / |V| = 1e7 about 1e-8 is left;
 * nothing is lost for |E| <= |V|.
 * PGBP_ERR_STATE without a family table.  PGBP_ERR_INVALID with NOTHING changed (the previous noise stays in force) and a text
 * that names the entry for: a family index out of range, a family that is not a tip family, a family listed twice, a value
 * that is not finite, an asymmetric sigma_e, a negative scale, se2 or diagonal entry of sigma_e; and when the correction of the
 * largest noisy cluster -- its record plus two p x (2p + 1) systems -- needs more than the 160 KB of LDS.  Up to six copies
 * (for a univariate per-site batch se2 once more as [entry][site]) and one stream synchronisation.
 * pgbp_lg_tip_noise_count: the number of noisy tips in force (0: none; -1: no family table). */
int pgbp_lg_set_tip_noise(pgbp_engine* e, int32_t n, const int32_t* family, const double* scale, const double* sigma_e,
                          const double* se2, int32_t per_site);
int32_t pgbp_lg_tip_noise_count(pgbp_engine* e);
/* PER-SITE MISSING TIPS of a UNIVARIATE BATCH.  child_mask of pgbp_lg_families is one missingness pattern for all sites of the
 * engine; a real batch (thousands of characters on one tree) lacks another set of species at almost every site.  At p = 1 a
 * tip that is not observed is exactly a family the fill skips -- its factor is 1 -- with no change of scopes or of the cluster
 * graph, so the pattern may depend on the site:
 *   missing [n_sites][n_rows], nonzero = the tip with that data row is NOT observed at that site; NULL clears the mask (so does
 *           a mask without a nonzero entry).  The call REPLACES the previous mask.
 * ACCEPTED ONLY ON A THREAD-PER-SITE ENGINE, as pgbp_lg_gradient_sites: p = 1, every belief of at most 2 variables, at least 8
 * sites; anything else is PGBP_ERR_INVALID before anything changes, and the text points to pgbp_patterns (one engine per
 * pattern), which stays the route at p > 1.  Clearing (NULL) is accepted on every engine with a family table, whatever its
 * shape: there is nothing to clear there and the call returns PGBP_OK.  PGBP_ERR_STATE without a family table.
 * Takes effect as pgbp_lg_set_shifts does: at the next pgbp_lg_assignfactors or pgbp_enqueue_loglik_lg; beliefs and factors
 * are not refilled by this call.  The mask survives pgbp_lg_set_edges, pgbp_lg_set_shifts, pgbp_lg_set_tip_noise and
 * pgbp_lg_set_data; a new pgbp_lg_setup clears it.  An engine borrowed from a pgbp_group or pgbp_patterns takes the call like
 * any other; there is no group-level call.
 * REFUSED with PGBP_ERR_INVALID and NOTHING changed (the previous mask stays in force; the text names the site and the row):
 * a nonzero entry at a row that belongs to no tip family (child_pos < 0, a data row, a parent edge); a nonzero entry at a row
 * whose tip the set-up's child_mask already skips at every site (the text names the family; harmless, but most likely not
 * what was meant); a site left with no observed tip (where tip families share a data row a masked row hides every one of them:
 * observed tips are counted in families).
 * DATA: the value at a masked entry is never used.  The setter stores 0.0 there in the engine's copies of the data
 * (pgbp_lg_get_data returns it), and while a mask is in force pgbp_lg_set_data accepts any value, finite or not, at a masked
 * entry and stores 0.0.  An entry that a later mask no longer covers keeps that 0.0 until new data are given.
 * pgbp_lg_simulate is left alone: with write_data it writes every statically observed row; a value written under the mask is
 * ignored like any other.
 * DEVICE: the mask is kept as bit-packed words uint64 [n_rows][W], W = ceil(n_sites / 64), bit (s & 63) of word s >> 6 = site
 * s: a wavefront of 64 consecutive sites reads at most two words of a row.  Every fill, after its shift and noise
 * corrections, is followed by csrc/pgbp_sitemiss.hip: lanes = sites, 256 sites per workgroup, one row of workgroups per
 * cluster that holds a tip family masked at some site (a sparse list the setter builds).  A thread whose site masks no family
 * of its cluster stores nothing -- that record keeps the fill's bytes --; one whose site does RECOMPUTES the cluster's record
 * (J, h, g, with the shifts and the tip noise in force) from the family table without the masked families and writes it to
 * beliefs and, where the fill does, factors.  Recomputed, never subtracted: a cluster whose only family is the masked tip
 * holds exactly +0.0 in every entry, nothing depends on the stored placeholder, and no cancellation error remains.  One writer
 * per record, no atomics: the same bytes on every call.  Nothing is launched when no mask is set, and every call then returns
 * the bytes it returned before this call existed.
 * THE SWEEPS.  The lanes-are-sites calls read the CURRENT mask as they read the shifts and the noise:
 *   pgbp_lg_gradient_sites, pgbp_lg_shift_scan_sites, pgbp_lg_edge_gradient_sites: a masked (family, site) is a skipped family
 *     with that call's convention for one (it adds nothing; jump / information NaN, lr 0; derivatives and dshift 0);
 *   pgbp_lg_loo_sites: a masked (tip, site) has mean, var and lpd NaN and info PGBP_INFO_NOT_OBSERVED, and adds nothing to
 *     total (unlike a tip that is not determined, which makes total NaN);
 *   pgbp_lg_impute_count / _families / _sites: the list is the statically missing tips plus every tip masked at some site, in
 *     family order (predicted mask 1).  At a site where such a tip is observed mean and var are NaN and info is
 *     PGBP_INFO_NOT_OBSERVED (there is nothing to impute); at a masked site the prediction is the existing
 *     closed form from the cluster's belief, which then does not contain the tip.
 *   pgbp_moments_sites, pgbp_sample_posterior_sites and pgbp_posterior_cov_sites read beliefs only and need no change.
 * Where every tip below an internal node is masked at a site, scopes do not shrink as they would in the reference: the cluster
 * {node, parent} then sends the message q^2 j - (q j)^2 / j, zero up to an ulp and possibly slightly negative.  It is added to
 * a positive precision and is harmless; the scan reports the edge above such a clade as not identified at that site
 * (H = j - j C j is 0 to rounding).
 * THE GENERAL SWEEPS cannot honour the mask and would be silently wrong: while one is in force pgbp_lg_gradient(_noise),
 * pgbp_lg_edge_gradient, pgbp_lg_shift_scan, pgbp_lg_loo, pgbp_lg_impute and pgbp_bm_exact_stats return PGBP_ERR_INVALID
 * before anything else happens (layout, pool and outputs untouched), the text naming the _sites call to use.
 * pgbp_lg_get_site_missing: the mask in force as bytes [n_sites][n_rows] (0 / 1), zeros when none.
 * pgbp_lg_site_missing_count: the number of masked (row, site) pairs (0: no mask; -1: no family table). */
#define PGBP_INFO_NOT_OBSERVED (-2)
int pgbp_lg_set_site_missing(pgbp_engine* e, const uint8_t* missing);
int pgbp_lg_get_site_missing(pgbp_engine* e, uint8_t* missing);
int32_t pgbp_lg_site_missing_count(pgbp_engine* e);
/* pgbp_lg_gradient with one more output (NULL allowed: then exactly pgbp_lg_gradient):
 *   dsigma_e [sites][p*p] column-major, symmetric: sum over the noisy tip families of scale_f G_V(f), G_V formed with
 *            j = (V_OO + E_OO)^-1, so that d loglik = tr(dsigma_e dSigma_e); zeros when no noise is set.
 * It is one more block of the family slot (a coefficient scale_f beside those of the rates), added by the same fixed tree
 * as dR: no atomics, two calls return the same bytes. */
int pgbp_lg_gradient_noise(pgbp_engine* e, int32_t site_begin, int32_t site_end, double* dR, double* dmu, double* dalpha,
                           double* dtheta, double* dsigma_e, int32_t* info);
/* pgbp_lg_gradient_noise for the sites of a UNIVARIATE BATCH, lanes = sites (csrc/pgbp_grad_uni.hip): the same quantities as
 * documented for pgbp_lg_gradient, in the layout of pgbp_lg_gradient_noise at p = 1 -- dR [sites][n_rates], then one double per
 * site in dmu, dalpha, dtheta and dsigma_e (NULL allowed).  Accepted only on a thread-per-site engine: p = 1, every belief of
 * at most 2 variables, at least 8 sites; anything else is PGBP_ERR_INVALID before any launch, the reason named.  The state
 * errors and range checks are those of pgbp_lg_gradient.
 * A thread walks a block of 64 consecutive families for its one site and solves each family's cluster (0, 1 or 2 variables)
 * in closed form; the blocks' partial sums are added in index order by a second kernel.  No atomics and every sum in a fixed
 * order: two calls return the same bytes, and a site's bytes do not depend on the site range it is asked in.  The call reads
 * the beliefs in the layout they are in (site-minor from 64 sites on) and converts nothing: pgbp_layout is the same before and
 * after.  Shared and per-site parameters, the shifts and the tip noise in force are read as pgbp_lg_gradient reads them.
 * The partial sums of a chunk of sites at a time (whole workgroups of 256 sites) are bounded by
 * pgbp_sites_sweep_scratch_limit, 256 MB unless it is set; the bytes do not depend on the chunks.
 *   info[site]: 0, or the 1-based index of a cluster that is not positive definite (or whose family has a variance that is
 *   not positive) at that site: the site's outputs are then NaN, every other site is unaffected.
 * Values agree with pgbp_lg_gradient to rounding (the closed forms add in another order), not to the byte. */
int pgbp_lg_gradient_sites(pgbp_engine* e, int32_t site_begin, int32_t site_end, double* dR, double* dmu, double* dalpha,
                           double* dtheta, double* dsigma_e, int32_t* info);
/* SCAN OF EVERY EDGE FOR A MEAN SHIFT from the CURRENT beliefs, for sites [site_begin, site_end): per family the maximum-
 * likelihood displacement of the child's conditional mean, its observed information and the likelihood-ratio statistic, under
 * the parameters the engine kept from the last pgbp_lg_assignfactors and the shifts in force.  EXACT ONLY WHEN THE BELIEFS ARE
 * CALIBRATED (postorder AND preorder) ON A CLIQUE TREE under those parameters and shifts; the call does not verify that.
 * The log-likelihood is quadratic in a displacement d (r = x_child - sum_k qc_k x_k - w - d).  In the notation of
 * pgbp_lg_edge_gradient (O = child_mask[f], mo = |O|, j = V_OO^-1, e = E[r], g_w = j e) and with C = Cov(r | data), the
 * covariance of the residual under the cluster's belief WITHOUT the e e' term:
 *     H_f = j - j C j  (mo x mo, the observed information of d: no data value enters it),
 *     dhat = H_f^-1 g_w,      lr = 2 (ll(dhat) - ll(0)) = g_w' H_f^-1 g_w.
 * A shift s_k on parent edge k enters as gamma_k s_k: shat_k = dhat / gamma_k, its information is gamma_k^2 H_f and lr is the
 * same for every parent edge of a hybrid.  With shifts set, e is the residual at the current shifts: dhat is the INCREMENT to
 * that edge's shift and lr the gain of a jump there while the other shifts stay where they are.
 * The traits of O are taken in index order by a Cholesky factorisation with a skip: a trait whose pivot, given the kept
 * traits before it, is not greater than min_info * j_ii is NOT IDENTIFIED (no tip below observes it, or the data leave the
 * prior untouched) and is dropped, row and column; dhat and lr are then those of the displacement restricted to the kept
 * traits.  H_f is formed from C itself, not by taking e e' back out of the gradient's M: its bytes do not depend on the data.
 * Outputs, site-major; any of the four may be NULL, not all four:
 *   jump        [sites][n_families][p]     dhat embedded in the p traits; NaN at a trait outside O or not identified;
 *   lr          [sites][n_families]        the gain; 0 when no trait is identified;
 *   identified  [sites][n_families]        bit t set: trait t is kept;
 *   information [sites][n_families][p][p]  H_f at the kept traits, symmetric; NaN elsewhere.
 *   A root-prior family has no edge: jump, lr and information NaN, identified 0.  A family the factor fill skips
 *   (child_mask == 0): jump and information NaN, lr 0, identified 0.
 *   info [sites] (may be NULL): as pgbp_lg_edge_gradient's; that site's outputs are all NaN (identified 0), other sites are
 *   unaffected.
 * Device (csrc/pgbp_scan.hip): the frame of pgbp_lg_edge_gradient -- one workgroup per (family, site), 64 threads while every
 * family's cluster has at most 64 variables, else 256, the cluster solved in LDS -- no reduction, no atomics on doubles, every
 * sum in a fixed index order: the same bytes on every call and for every split of the site range.  Device copies of the
 * outputs of a chunk of sites at a time (256 MB at most), one stream synchronisation per call.  Read-only on the beliefs;
 * every layout, as pgbp_lg_edge_gradient.
 * Fails before any launch, the outputs untouched, with PGBP_ERR_STATE without a family table or before the first
 * pgbp_lg_assignfactors, with PGBP_ERR_INVALID for p > 64 (as soon as the table is known), for a site range out of bounds, for
 * all four outputs NULL, for min_info outside [0, 1), for a family whose cluster has more than 128 variables (the message
 * names the family and the cluster), and when the LDS need -- the largest cluster's working matrix plus p x (2p + 1) +
 * 3 p x p + 5 p doubles of family scratch and, in the packed layout, the plain copy of a record -- exceeds 160 KB. */
int pgbp_lg_shift_scan(pgbp_engine* e, int32_t site_begin, int32_t site_end, double min_info, double* jump, double* lr,
                       uint64_t* identified, double* information, int32_t* info);
/* LEAVE-ONE-OUT predictive moments of every tip from the CURRENT beliefs, for sites [site_begin, site_end): for each tip family
 * of the table given to pgbp_lg_setup (child_pos < 0, data_row >= 0, at least one observed trait: O = child_mask, o = |O|), the
 * distribution of the tip's observed values y_O given the data of all OTHER tips, with the parameters the engine kept from the
 * last pgbp_lg_assignfactors (shared or per site: a per-site engine returns each site's own prediction).
 * THE RESULT IS THE EXACT LEAVE-ONE-OUT PREDICTIVE ONLY WHEN THE BELIEFS ARE CALIBRATED (postorder AND preorder) ON A CLIQUE TREE
 * UNDER THE PARAMETERS OF THE LAST pgbp_lg_assignfactors; the call does not verify that.  On a loopy cluster graph the same sweep
 * on the beliefs of a CONVERGED calibration is the Bethe approximation of it; before convergence it is neither.
 * Per tip family (notation of pgbp_lg_params): the tip's factor is N(y_O; u + w, V) with u = (sum_k qc_k x_k)_O the parents'
 * contribution (a fixed-root parent: its constant), w = (sum_k wc_k theta)_O, V = (sum_k vc_k R[colour_k])_OO.  With
 * m_u = E[u], S = Cov(u) from the cluster's J^-1 h and J^-1 (S = 0 when no parent is in scope) and r = y_O - w - m_u:
 *     D = V - S,   cov = V D^-1 V,   mean = y_O - V D^-1 r,
 *     lpd = -(o log 2pi + 2 log det V - log det D + r' D^-1 r) / 2      (the log predictive density of y_O).
 * pgbp_lg_loo_count: the number n_tip of tip families (-1: no family table); pgbp_lg_loo_families: their indices into the
 * family table, in order -- the order of every output.  Outputs, site-major:
 *   mean  [sites][n_tip][p]    NaN at the unobserved traits; may be NULL;
 *   cov   [sites][n_tip][p*p]  column-major, symmetric, both triangles written, NaN rows / columns at the unobserved traits;
 *                              may be NULL;
 *   lpd   [sites][n_tip];
 *   total [sites]: the sum of lpd in tip-family order (thread r of 256 adds the tips r, r + 256, ... in order, the partial sums
 *         are added by a fixed tree); may be NULL;
 *   info  [sites][n_tip] (may be NULL): 0; 1 when D (or V) is not positive definite -- the other data leave u undetermined: an
 *         improper root with no other informative tip, an improper cavity; a pivot of D's factorisation that is not above
 *         2^-40 times V's diagonal entry counts as not positive (D is formed by cancellation: below that it is rounding
 *         noise), as does a cluster whose belief is the constant 1 --; or 1 + PosDefException.info of the cluster.  Where
 *         info is not 0 that tip's mean, cov and lpd are NaN and so is the site's total; other tips and sites are unaffected.
 * Device (csrc/pgbp_loo.hip): one workgroup per (tip family, site) solves the family's cluster in LDS (the solve of
 * pgbp_moments), forms V, D and the right-hand sides [V | r], factorises D and V by Cholesky and writes its outputs; a second
 * kernel adds the site's total.  No atomics, every sum in index order: two calls return the same bytes, and the result for a
 * site does not depend on which other sites are in the call.  The device copies of the outputs of a chunk of sites at a time
 * (256 MB at most; pgbp_loo_scratch_limit: that bound in doubles, process-wide, <= 0 restores the default -- the results do
 * not depend on the chunks).  Read-only on the beliefs; every layout (a site-minor univariate batch is converted to the plain
 * layout first, as pgbp_bm_exact_stats does); one stream synchronisation per call.
 * Fails before any launch with PGBP_ERR_STATE without a family table or before the first pgbp_lg_assignfactors, with
 * PGBP_ERR_INVALID for a site range out of bounds, for lpd NULL, for a family whose cluster has more than 128 variables
 * (the message names the family and the cluster), and when the largest cluster's working matrix plus the 3 p x p scratch
 * exceed the 160 KB of LDS -- the limits of pgbp_lg_gradient, taken as there over the clusters of ALL families of the table:
 * an engine serves both sweeps or neither (the tip families' own clusters are small; the limit is conservative for them).
 * A table without tip families returns PGBP_OK and writes only total = 0. */
int32_t pgbp_lg_loo_count(pgbp_engine* e);
int     pgbp_lg_loo_families(pgbp_engine* e, int32_t* fam);
int     pgbp_lg_loo(pgbp_engine* e, int32_t site_begin, int32_t site_end, double* mean, double* cov, double* lpd,
                    double* total, int32_t* info);
void    pgbp_loo_scratch_limit(int64_t doubles);
/* pgbp_lg_shift_scan, pgbp_lg_edge_gradient and pgbp_lg_loo for the sites of a UNIVARIATE BATCH, lanes = sites
 * (csrc/pgbp_fam_uni.hip; the shared closed forms in csrc/pgbp_fam_uni_dev.hpp): each is the p = 1 case of the statement
 * documented for the general call, with its conventions for root-prior families, skipped families (child_mask == 0), entries
 * k >= n_parents and failed sites.  Accepted only on a thread-per-site engine, as pgbp_lg_gradient_sites: p = 1, every belief
 * of at most 2 variables, at least 8 sites; anything else is PGBP_ERR_INVALID before any launch, the outputs untouched, the
 * reason naming the general call to use instead.  The state errors and range checks are those of pgbp_lg_gradient_sites.
 * A workgroup is 256 consecutive sites; a thread walks a block of 64 consecutive families (tip families for the leave-one-out
 * sweep) for its one site and solves each family's cluster (0, 1 or 2 variables) in closed form.  The calls read the beliefs
 * in the layout they are in (site-minor from 64 sites on) and convert nothing: pgbp_layout is the same before and after, and
 * the next calibration finds the layout it left.  Shared and per-site parameters, the shifts and the tip noise in force are
 * read as the general calls read them.  No atomics, every sum in a fixed order: two calls return the same bytes, and a site's
 * bytes depend neither on the site range nor on the chunks it came in.  Values agree with the general calls to rounding (the
 * closed forms add in another order), not to the byte.
 * OUTPUTS ARE SITE-MINOR: one row of (site_end - site_begin) values per (family[, entry]) -- the transpose of the general
 * calls' tables.  The rows of a chunk of sites at a time go through device scratch (256 MB at most, whole workgroups of 256
 * sites; pgbp_sites_sweep_scratch_limit: that bound in doubles, process-wide, <= 0 restores the default -- the results do not
 * depend on the chunks) and are copied into the caller's rows by strided copies; one stream synchronisation per call.
 * pgbp_lg_shift_scan_sites: with j = 1 / V, C = u' Sigma u, g_w = j e and H = j - j C j (formed from C), a family is
 *   identified iff H > min_info * j; then jump = g_w / H, lr = g_w^2 / H.
 *   jump, lr, information [n_families][sites] (each may be NULL): jump and information NaN where the family is not identified,
 *       is skipped or is a root-prior family; lr 0 where it is not identified or skipped, NaN for a root-prior family.
 *   top_lr, top_family [sites] (may be NULL; not all five NULL): the largest lr of the site over the families that have at
 *       least one parent, are identified and whose lr is finite, and the family that has it -- ties go to the lowest family
 *       (a thread keeps its block's best with a strict >, a second kernel folds the blocks in index order with a strict >).
 *       A site with nothing identified: -inf and -1.  With only these two asked for no table is allocated or copied.
 *   info [sites] (may be NULL): as pgbp_lg_shift_scan's; that site's tables and top_lr are NaN, its top_family -1.
 *   min_info outside [0, 1) is PGBP_ERR_INVALID.
 * pgbp_lg_edge_gradient_sites: dlength, dgamma [n_families][K][sites], dshift [n_families][sites] (any may be NULL, not all
 *   three), info [sites] (may be NULL): the quantities of pgbp_lg_edge_gradient; dgamma carries the s_k g_w term of a shift.
 * pgbp_lg_loo_sites: for the tip families of pgbp_lg_loo_families, in that order: with S = Var(u) over the cluster parents
 *   and D = V - S, the prediction is determined iff D > 2^-40 V and V > 0; var = V^2 / D, mean = y - V r / D,
 *   lpd = -(log 2pi + 2 log V - log D + r^2 / D) / 2.
 *   mean, var [n_tip][sites] (may be NULL), lpd [n_tip][sites] (required), info [n_tip][sites] (may be NULL; the codes of
 *   pgbp_lg_loo), total [sites] (may be NULL): the per-block partial sums of lpd (blocks of 64 tips, added in tip order) added
 *   in block order by a second kernel -- another order than pgbp_lg_loo's, so the two totals agree to rounding.  NaN where
 *   a tip of the site is not determined. */
int  pgbp_lg_shift_scan_sites(pgbp_engine* e, int32_t site_begin, int32_t site_end, double min_info, double* jump, double* lr,
                              double* information, double* top_lr, int32_t* top_family, int32_t* info);
int  pgbp_lg_edge_gradient_sites(pgbp_engine* e, int32_t site_begin, int32_t site_end, double* dlength, double* dgamma,
                                 double* dshift, int32_t* info);
int  pgbp_lg_loo_sites(pgbp_engine* e, int32_t site_begin, int32_t site_end, double* mean, double* var, double* lpd,
                       double* total, int32_t* info);
void pgbp_sites_sweep_scratch_limit(int64_t doubles);
/* pgbp_lg_optimum_scan_sites: every edge scanned for a SHIFT OF THE OPTIMUM OF ITS CLADE under PGBP_LG_OU, for the sites of a
 * univariate batch on a tree, lanes = sites (csrc/pgbp_optscan_uni.hip; the plan in csrc/pgbp_optscan_host.cpp), in the frame
 * of the three calls above.  For the edge above family v the question is an increment delta added to the optimum of EVERY edge
 * of clade(v) -- that edge and all edges below it, whatever regimes they carry (the nested-shift parametrisation).  The
 * log-likelihood is exactly quadratic in delta, so the calibrated beliefs -- at the parameters, shifts, tip noise, painted
 * optima and per-site mask in force -- hold the exact ML increment and its likelihood ratio of every edge.  With j = 1 / V
 * (tip noise included), kappa = wc j and e = E[r | data] of a family (the offset with the painted optima), and over the child
 * families c of v that are not skipped at the site, in index order (B = S = G = K = 0 at a tip):
 *     B_v = sum_c [(kappa_c + B_c) rho_c - kappa_c qc_c]        S_v = sum_c [S_c + (kappa_c + B_c)^2 tau_c]
 *     G_v = sum_c [G_c + kappa_c e_c]                           K_v = sum_c [K_c + wc_c kappa_c]
 *   rho_c = Cov(x_c, x_v) / Var(x_v), tau_c = Var(x_c) - Cov(x_c, x_v)^2 / Var(x_v) from the posterior of c's own cluster
 *   (0 for a tip).  Then g_v = G_v + kappa_v e_v, Kt_v = K_v + wc_v kappa_v, a = kappa_v + B_v, b = -kappa_v qc_v,
 *     Var_v = a^2 Var(x_v) + 2 a b Cov(x_v, x_u) + b^2 Var(x_u) + S_v   (a tip: b^2 Var(x_u); no x_u terms under the fixed root)
 *   and H_v = Kt_v - Var_v.  Family v is identified iff H_v > min_info Kt_v; then delta = g_v / H_v, lr = g_v^2 / H_v,
 *   information = H_v (se = 1 / sqrt(H_v)).  A family the fill skips at a site (child_mask == 0, a tip masked at that site)
 *   contributes nothing and is no candidate there.
 * One launch per height of the family tree, from the tips up (a tip has height 0, any other family 1 + the largest height of
 * its child families); a thread owns one (family of that height, site) and gathers four numbers per child family.
 *   delta, lr, information [n_families][sites] (each may be NULL): delta and information NaN where the family is not
 *       identified or skipped, lr 0 there; all three NaN for a root-prior family.
 *   top_lr, top_family [sites] (may be NULL; not all five NULL): the largest lr over the identified families that have a
 *       parent, and the first family that has it; -inf and -1 when nothing is identified; NaN and -1 at a failed site.  With
 *       only these two asked for no table is allocated on the host or copied.
 *   info [sites] (may be NULL): the 1-based index of the first cluster in preorder of schedule tree 0 whose conditional
 *       precision is not positive definite at that site (the validity pass of pgbp_sample_posterior_sites), 0: none; such a
 *       site is NaN everywhere.
 * Refused before any launch, outputs, layout, pool and settings untouched: what pgbp_lg_gradient_sites refuses; a
 * Brownian-motion fill (wc = 0: use pgbp_lg_shift_scan_sites); no topology (PGBP_ERR_STATE: call pgbp_lg_set_topology); a
 * family with two or more parents (named); min_info outside [0, 1); a scratch limit below what one workgroup of 256 sites
 * takes -- 256 (n_families (4 + tables + 1 with top) + ...) doubles, the text names the number that suffices.  Painted optima
 * are read, not refused; an improper root is accepted.  No atomics, contraction off, every sum in a fixed order: two calls,
 * every split of the site range, every chunking and both layouts give the same bytes.
 * _timed (measurement only): ms4 = {validity pass, height launches, top fold, copies} in milliseconds, the stream drained
 * after every phase; launches (may be NULL): the number of height launches of the call. */
int  pgbp_lg_optimum_scan_sites(pgbp_engine* e, int32_t site_begin, int32_t site_end, double min_info, double* delta, double* lr,
                                double* information, double* top_lr, int32_t* top_family, int32_t* info);
int  pgbp_lg_optimum_scan_sites_timed(pgbp_engine* e, int32_t site_begin, int32_t site_end, double min_info, double* delta,
                                      double* lr, double* information, double* top_lr, int32_t* top_family, int32_t* info,
                                      double* ms4, int32_t* launches);
/* PER-SITE CLADE SHIFTS OF THE OPTIMUM under OU, for a thread-per-site engine (p = 1, every belief of at most 2 variables, at
 * least 8 sites, either layout) on a tree with pgbp_lg_set_topology done: the nested-shift parametrisation that
 * pgbp_lg_optimum_scan_sites scans.  At site s the optimum of every edge of clade(family[j][s]) -- the parent edge of that
 * family and all edges below it -- gains delta[j][s], j < n_slots; family and delta are [n_slots][n_sites], family -1 marks an
 * empty slot (its delta is not read).  The optimum of an edge is theta (or its painted value, pgbp_lg_set_optima) plus the
 * deltas of the site's slots whose clade holds it, added in slot order.  n_slots = 0 clears the setting.
 * Refused with PGBP_ERR_INVALID, the previous setting left in force: another engine (the wording of
 * pgbp_lg_set_site_missing), a family with two or more parents, a family out of range, a root-prior family (no parent edge),
 * a family twice at one site (the reason names site and family), a delta that is not finite; PGBP_ERR_STATE without a table or
 * a topology.  The setting takes effect at the next fill (pgbp_lg_assignfactors): a correction of its own after the shift and
 * noise corrections (csrc/pgbp_shift.hip), lanes = sites, over the clusters that hold a family inside some site's clade; a
 * thread whose site has no slot covering the cluster stores nothing.  Nothing is launched without a setting, and under BM
 * (wc = 0) it has no effect, byte for byte.  It survives pgbp_lg_set_edges, _set_shifts, _set_optima, _set_tip_noise,
 * _set_site_missing and _set_data; a new pgbp_lg_setup or pgbp_lg_set_topology clears it.
 * pgbp_lg_optimum_scan_sites honours it (the next scan finds the next increment).  Every call that refuses painted optima,
 * and pgbp_lg_gradient, pgbp_lg_gradient_sites and pgbp_lg_gradient_sites_optima, refuse while a setting is in force under OU
 * (PGBP_ERR_INVALID, before any launch, naming this setter).
 * _update_: the deltas alone [n_slots][n_sites] into the buffers of the setting in force, without allocation; the families are
 * not checked again.  _slots: the number of slots in force (0: none; -1: no family table).  _get_: the setting in force.
 * _score_: for every slot of every site of [site_begin, site_end) the scan's g_v, H_v and Kt_v at that site's own family v --
 * g the exact derivative of the log-likelihood in delta_j, information the diagonal of the joint information -- as
 * [n_slots][sites] rows; info [sites] and min_info as in pgbp_lg_optimum_scan_sites, whose frame and height launches it shares.
 * An empty slot and a failed site are NaN; a slot with H_v <= min_info Kt_v is not identified: information NaN there, as the
 * scan reports it.  The rows stay in scratch; one thread per (slot, site) picks row family[slot][site]. */
int  pgbp_lg_set_clade_shifts_sites(pgbp_engine* e, int32_t n_slots, const int32_t* family, const double* delta);
int  pgbp_lg_update_clade_shifts_sites(pgbp_engine* e, const double* delta);
int32_t pgbp_lg_clade_shift_slots(pgbp_engine* e);
int  pgbp_lg_get_clade_shifts_sites(pgbp_engine* e, int32_t* family, double* delta);
int  pgbp_lg_clade_shift_score_sites(pgbp_engine* e, int32_t site_begin, int32_t site_end, double min_info, double* g,
                                     double* information, double* kt, int32_t* info);
/* pgbp_moments, pgbp_sample_posterior and pgbp_lg_impute for the sites of a UNIVARIATE BATCH, lanes = sites
 * (csrc/pgbp_post_uni.hip): what is asked of a fitted batch -- the posterior moments of every belief, joint draws of all
 * ancestral states, the predictions of the tips without data -- in the frame of the three calls above.  Accepted and refused
 * as pgbp_lg_gradient_sites: a family table and parameters (PGBP_ERR_STATE otherwise), a site range inside the engine's, p = 1,
 * every belief of at most 2 variables, at least 8 sites; anything else is PGBP_ERR_INVALID before any launch, the outputs
 * untouched, the reason naming the general call to use instead.  A workgroup is 256 consecutive sites; a thread walks a block of
 * 64 table entries for its one site, everything in closed form.  The beliefs are read in the layout they are in and nothing is
 * converted: pgbp_layout is the same before and after and the pool keeps its bytes.  No atomics, every sum in a fixed order:
 * two calls return the same bytes, and a site's bytes depend neither on the site range nor on the chunks.  Values agree with
 * the general calls to rounding, not to the byte.  ALL OUTPUTS ARE SITE-MINOR ROWS of (site_end - site_begin) values; a chunk
 * of sites at a time goes through device scratch bounded by pgbp_sites_sweep_scratch_limit (whole workgroups of 256 sites, one
 * at least; the draws of pgbp_sample_posterior_sites are cut first); one stream synchronisation per call.
 * pgbp_moments_sites: the semantics of pgbp_moments for the n listed beliefs (beliefs == NULL: every cluster; sepset beliefs
 *   are allowed; an index out of range is PGBP_ERR_INVALID).
 *   mean [sum of dims][sites]            the variables of the listed beliefs, belief after belief;
 *   cov  [sum of m (m + 1) / 2][sites]   the upper triangle of Sigma = J^-1 in column order: S00, S01, S11; may be NULL;
 *   norm [n][sites]                      g + ((m log 2pi - log det J) + h'mu) / 2, log det J = log a (+ log of the Schur
 *                                        complement) -- the terms in this order;
 *   info [n][sites]                      may be NULL: 0, or PosDefException.info (that entry's mean, cov and norm are NaN).
 *   The all-zero belief (J = 0, h = 0) has mean Inf, norm g, cov NaN, info 0; a belief without variables has only norm = g.
 *   mean and norm NULL is PGBP_ERR_INVALID.
 * pgbp_sample_posterior_sites: the semantics documented for pgbp_sample_posterior -- S and R of a child cluster of schedule
 *   tree `tree`, x_R = J_RR^-1 (h_R - J_RS x_S) + L^-T z_R with L lower triangular in the child's variable order, z at S
 *   positions ignored, a 0-variable sepset an independent draw, a shared variable the same bits in every cluster that holds it,
 *   z = 0 the joint mean -- and its refusals, after those above: no schedule (PGBP_ERR_STATE), `tree` out of range, not a
 *   spanning clique tree, n_draws < 1, x NULL.  The same z gives pgbp_sample_posterior's draw to rounding.
 *   z, x [n_draws][pgbp_sample_size][sites]: the entry layout of pgbp_sample_posterior, transposed.
 *   z == NULL: the device generates the normals itself from `seed`:
 *     (r0, r1, r2, r3) = Philox4x32-10(counter = (entry, draw, absolute site, 1), key = (seed & 0xffffffff, seed >> 32)), the
 *     constants and the two 53-bit uniforms u1 (r0, r1), u2 (r2, r3) as documented for pgbp_lg_simulate;
 *     z = sqrt(-2 log u1) cos(2 pi u2), 2 pi = 6.283185307179586 (one normal per counter; the sine is dropped).
 *   The last counter word 1 keeps the stream disjoint from pgbp_lg_simulate's under the same seed.  The generator is
 *   stateless: the value of an (entry, draw, site) depends neither on the site range nor on the chunks.  With z != NULL the
 *   seed is not read.
 *   info [sites] (may be NULL): 0, or the 1-based index of the first cluster in preorder whose J_RR is not positive definite
 *   (pivot by pivot, in the order of R); all draws of that site are NaN, other sites keep their bytes.
 *   Device: a validity pass (a thread walks blocks of 64 clusters in preorder rank, the blocks folded in order), then one
 *   launch per preorder level, thread = site, the clusters of the level along grid.y, the draws in a loop; the at most five
 *   coefficients of a cluster's conditional are formed in registers by the launch that uses them -- no factor pool.
 * pgbp_lg_impute_sites: the p = 1 case of pgbp_lg_impute for the families of pgbp_lg_impute_families, in that order.  A listed
 *   tip observes nothing at p = 1: mean = E[u] + w, var = u' Sigma u + V over the cluster parents, with the shifts and the tip
 *   noise in force (a noisy tip predicts the observation).
 *   mean, var [n_listed][sites] (either may be NULL, not both), info [n_listed][sites] (may be NULL): the codes of
 *   pgbp_lg_impute -- 0; -1 where the static mask `predicted` is empty (a cluster parent lacks the trait: NaN); 1 when V is not
 *   positive or the cluster's belief is the constant 1; 1 + PosDefException.info of the cluster. */
int  pgbp_moments_sites(pgbp_engine* e, int32_t n, const int32_t* beliefs, int32_t site_begin, int32_t site_end, double* mean,
                        double* cov, double* norm, int32_t* info);
int  pgbp_sample_posterior_sites(pgbp_engine* e, int32_t tree, int32_t site_begin, int32_t site_end, int32_t n_draws,
                                 const double* z, uint64_t seed, double* x, int32_t* info);
int  pgbp_lg_impute_sites(pgbp_engine* e, int32_t site_begin, int32_t site_end, double* mean, double* var, int32_t* info);
/* pgbp_sample_posterior_sites with the stream drained after each phase (measurement only: tools/time_post_uni.py):
 * ms4[0 .. 3] = wall milliseconds of {validity pass, copy of z, level launches, copy of x}, summed over the chunks. */
int  pgbp_sample_posterior_sites_timed(pgbp_engine* e, int32_t tree, int32_t site_begin, int32_t site_end, int32_t n_draws,
                                       const double* z, uint64_t seed, double* x, int32_t* info, double* ms4);
/* CLOSED-FORM BM FIT OF EVERY SITE OF A UNIVARIATE BATCH, LANES = SITES (csrc/pgbp_exact_uni.hip): the family sweep of
 * pgbp_bm_exact_stats (src/calibration.jl:440-499) in the frame of the calls above, with the per-site mask of missing tips
 * (pgbp_lg_set_site_missing), the shifts in force and the root's posterior mean in the same call.  THE CALLER GUARANTEES, as
 * for pgbp_bm_exact_stats, THAT THE BELIEFS WERE CALIBRATED ON A CLIQUE TREE UNDER A BROWNIAN MOTION WITH R = 1 AND AN IMPROPER
 * ROOT; the call does not verify it.
 * Per (family f, site) that is not skipped: t_f = sum_k gamma_k^2 length_k (:459); r = x_child - sum_k gamma_k x_k - d_f, with
 * x_child the tip's data value when the child is a tip and d_f the displacement of the shifts on the family's parent edges;
 * e = E[r | data] and C = Var(r | data) from the calibrated belief of the family's cluster (0, 1 or 2 variables, closed form);
 * the family adds e^2 / t_f to num and 1 - C / t_f to den.  Skipped, as the reference and pgbp_bm_exact_stats skip them: a
 * root-prior family, t_f == 0, child_mask == 0, a tip whose parent holds nothing in scope, a cluster without variables; and a
 * tip the per-site mask says is not observed at this site.  The scopes are those of the complete data: an internal family whose
 * whole clade is masked at a site stays in the sweep and adds e = 0, C = t_f, that is 0 to both sums.  den is then the number
 * of tips the site observes less one, to rounding, and num / den the REML estimate of the rate on those tips.
 *   num, den [sites]   required;
 *   mu  [sites]        may be NULL: the posterior mean of variable root_pos of belief root_belief -- mu_hat of :435-437;
 *   info [sites]       may be NULL: 0, or the 1-based index of the lowest cluster the site needed (root_belief with mu) that is
 *                      not positive definite; that site's num, den and mu are NaN, its neighbours keep their bytes.  A needed
 *                      cluster whose belief is the constant 1 gives NaN with info 0, as in pgbp_bm_exact_stats.
 * Device: a workgroup is 256 consecutive sites, grid.y a block of 64 consecutive families; a thread walks its block in index
 * order for its one site and writes its two sums, each started from 0.0, to partial[block][2][site]; a second kernel adds the
 * blocks in block order (and forms mu).  No atomics, no LDS, no barrier, contraction off: two calls return the same bytes, and a
 * site's bytes depend neither on the site range nor on the chunks (pgbp_sites_sweep_scratch_limit).  The pool is read in the
 * layout it is in: pgbp_layout and the pool's bytes are the same before and after.  One stream synchronisation per call.
 * Refused before any launch -- outputs, layout and pool untouched --: as pgbp_lg_gradient_sites, in its order (no table, no
 * parameters: PGBP_ERR_STATE; the site range; num or den NULL; more than one trait, a belief above 2 variables, fewer than 8
 * sites, an engine off the thread-per-site kernels: the text names pgbp_bm_exact_stats), then with PGBP_ERR_INVALID when the
 * last pgbp_lg_assignfactors was an Ornstein-Uhlenbeck fill; when tip noise is in force (the variance is then not proportional
 * to the rate: fit_sites_lg); for a family whose parent is the fixed root (the wording of pgbp_bm_exact_stats); for a tip family
 * with more than one parent (the reference raises there: a hybrid tip); and for mu != NULL with root_belief or root_pos out of
 * range. */
int  pgbp_bm_exact_stats_sites(pgbp_engine* e, int32_t site_begin, int32_t site_end, int32_t root_belief, int32_t root_pos,
                               double* num, double* den, double* mu, int32_t* info);
/* EVOLUTIONARY RATE MATRIX BETWEEN THE SITES OF A UNIVARIATE BATCH (csrc/pgbp_rate_uni.hip): the cross-site form of the call
 * above -- evol.vcv / ratematrix, the evolutionary correlations, phyl.pca -- for the sites [row_begin, row_end) against the
 * sites [col_begin, col_end) of a thread-per-site engine whose beliefs are CALIBRATED UNDER THE FACTORS OF R = 1, mu = 0 WITH AN
 * IMPROPER ROOT.  With e_fs = E[r_f | data of site s] and t_f as above, and the same observed tips at every site,
 *   gram[a][b] = (Y'PY)_ab = sum_f e_fa e_fb / t_f        (P: the projected precision of the tips)
 * whose diagonal is num of the call above; R_hat_ab = gram[a][b] / sqrt(den_a den_b) (den_a = den_b = tips - 1).
 *   gram [row_end - row_begin][col_end - col_begin]  required, row-major;
 *   den, mu, info [rows] then [cols]                 each may be NULL; the values of pgbp_bm_exact_stats_sites (den to the byte).
 * A site whose info is not 0 has NaN in its whole row or column of gram and in its den and mu; every other entry keeps its bytes.
 * Device, per chunk of families: rate_uni_resid, the frame of the sweep above, stores U[family][site] = e / sqrt(t_f) (+0.0 for
 * a skipped family and for the rows that pad the last family to a multiple of 4) and the block's den partial and mark, folded
 * in block order across the chunks; rate_uni_syrk adds U'U to the device-resident gram block on the matrix cores
 * (v_mfma_f64_16x16x4_f64): a workgroup of four wavefronts per 128 x 128 tile, accumulators in registers, the family axis walked
 * in index order 4 families per step through LDS slabs of 16 families.  No atomics, no split over the family axis, contraction
 * off: an entry sees the same sequence of steps whatever the ranges of the query, its tile and the chunks, so two calls, a query
 * cut into blocks, and the transposed query return the same bytes, and gram of a square query is symmetric to the byte (its
 * tiles wholly below the diagonal are copied from their mirror images, which have the bytes the update would have formed).
 * Scratch: the U rows of a chunk -- whole blocks of 64 families (one at least) over all row and column sites -- are bounded by
 * pgbp_sites_sweep_scratch_limit; the gram block, rows x cols doubles, is allocated outside that limit (PGBP_ERR_HIP with the
 * call's name when it does not fit: tile a large matrix through the ranges).  The pool is read in the layout it is in.
 * Refused before any launch -- outputs, layout and pool untouched --: as pgbp_bm_exact_stats_sites in its order (either range
 * outside the sites; gram NULL; not a thread-per-site engine: the text names pgbp_bm_exact_stats), then a per-site mask in
 * force (pgbp_lg_set_site_missing: a cross-site estimate needs the same observed tips at both sites; a shared child_mask is
 * fine), an Ornstein-Uhlenbeck fill, tip noise, a fixed-root parent, a leaf with two parents, and with mu the root out of range.
 * _timed: ms3 = {residual rows, rank-k update, copies} in milliseconds, the stream drained after every phase. */
int  pgbp_bm_rate_matrix_sites(pgbp_engine* e, int32_t row_begin, int32_t row_end, int32_t col_begin, int32_t col_end,
                               int32_t root_belief, int32_t root_pos, double* gram, double* den, double* mu, int32_t* info);
int  pgbp_bm_rate_matrix_sites_timed(pgbp_engine* e, int32_t row_begin, int32_t row_end, int32_t col_begin, int32_t col_end,
                                     int32_t root_belief, int32_t root_pos, double* gram, double* den, double* mu, int32_t* info,
                                     double* ms3);
/* THE RATE MATRIX OF A UNIVARIATE BATCH APPLIED TO A BLOCK OF VECTORS (csrc/pgbp_rate_apply_uni.hip): the operator of an
 * iterative consumer -- the leading phylogenetic principal components, a solve, a trace estimate -- where sites x sites doubles
 * are too many.  On the beliefs pgbp_bm_rate_matrix_sites expects (CALIBRATED UNDER R = 1, mu = 0 WITH AN IMPROPER ROOT), with
 * U[f][s] = e_fs / sqrt(t_f) its residual rows over the sites [site_begin, site_end) and n = site_end - site_begin,
 *   gv[j][a] = sum_f U[f][a] * (sum_b U[f][b] v[j][b])      = (gram of pgbp_bm_rate_matrix_sites(rows = cols = the range)) v_j
 * without the gram block being formed; R_hat v = gv / den.
 *   v    [n_vec][n]  required, vector-major (site-minor); 1 <= n_vec <= 64 (block a wider set over several calls);
 *   gv   [n_vec][n]  required;
 *   den, mu, info [n]   each may be NULL (mu NULL: the root is not read); the bytes pgbp_bm_rate_matrix_sites returns.
 * A SITE WHOSE info IS NOT 0 has no residual column, and U v mixes all the sites of the range: the call still returns PGBP_OK,
 * den and mu are NaN at that site only, and gv is NaN IN EVERY ENTRY (filled by the host after the last chunk) -- check info
 * once before iterating.  A sub-range is another operator (a principal block of the matrix), not a part of the same result.
 * Device, per chunk of whole 64-family blocks: rate_uni_resid / rate_uni_reduce of the rate matrix (one source, shared);
 * rate_apply_uv: W[f][j] = sum_b U[f][b] v[j][b], the site axis in index order 4 sites per v_mfma_f64_16x16x4_f64, a wavefront
 * per 16 families and all vectors; rate_apply_utw: Z[a][j] += sum_f U[f][a] W[f][j], the family axis in index order 4 families
 * per MFMA on top of what the chunks before left (the rule of rate_uni_syrk), a wavefront per 16 sites and all vectors.  Vectors
 * are padded to 16 with +0.0 vectors, sites to 16, the last family block with +0.0 rows.  One owner per tile, no split of a
 * contracted axis, no atomics, contraction off: two calls, every chunking (pgbp_sites_sweep_scratch_limit bounds U, W, Z and the
 * transposed v; a chunk is one block at least), the site-minor and the plain layout, and a vector sent alone or among 63 others
 * give the same bytes.  The pool is read in the layout it is in.  One stream synchronisation per call.
 * Refused before any launch -- outputs, layout and pool untouched --: as pgbp_bm_rate_matrix_sites in its order, with n_vec
 * outside 1 .. 64 and v or gv NULL (PGBP_ERR_INVALID) after the site range.
 * _timed: ms4 = {residual rows, U v, U' W, copies} in milliseconds, the stream drained after every phase. */
int  pgbp_bm_rate_apply_sites(pgbp_engine* e, int32_t site_begin, int32_t site_end, int32_t n_vec,
                              const double* v,      /* [n_vec][sites of the range], site-minor */
                              int32_t root_belief, int32_t root_pos,
                              double* gv,           /* [n_vec][sites of the range] */
                              double* den, double* mu, int32_t* info);   /* [sites], each may be NULL (mu: see root) */
int  pgbp_bm_rate_apply_sites_timed(pgbp_engine* e, int32_t site_begin, int32_t site_end, int32_t n_vec, const double* v,
                                    int32_t root_belief, int32_t root_pos, double* gv, double* den, double* mu, int32_t* info,
                                    double* ms4);
/* POSTERIOR COVARIANCE OF A UNIVARIATE BATCH WITH LANES = SITES (csrc/pgbp_cov_uni.hip): pgbp_posterior_cov (below) in the
 * frame of the three calls above, for the out-of-clique queries of a fitted batch -- the covariance of two ancestors that share
 * no cluster, the variance of a clade mean or of a contrast -- at every site at once.  The semantics are pgbp_posterior_cov's:
 * the same `tree`, size = pgbp_sample_size, entry layout and split of a cluster into S and R; with x = m + A z at one site
 *   c    [n_cols][size]                       the functionals, shared by the sites (wave-uniform on the device: scalar loads);
 *   w    [n_cols][size][sites] (may be NULL)  w = A'c; +0.0 at the S positions of non-root clusters;
 *   k    [n_cols][size][sites] (may be NULL)  k = A w = Cov(x, c'x | data); a variable held by several clusters has the same bits
 *                                             in every copy;
 *   gram [n_cols (n_cols + 1) / 2][sites] (may be NULL)  the upper triangle in column order (G00, G01, G11, ...: the packing of
 *                                             pgbp_moments_sites' cov) of G_ab = w_a . w_b = Cov(c_a'x, c_b'x | data), folded on
 *                                             the device: the sum over the entries is taken per block of 64 entries in index
 *                                             order (from 0.0), and the blocks are added in block order (from 0.0), as
 *                                             pgbp_lg_gradient_sites adds its partial sums;
 *   info [sites] (may be NULL)                the value of pgbp_sample_posterior_sites; w, k and gram of a site whose info is not
 *                                             0 are NaN, its neighbours keep their bytes.
 * w, k and gram may not all be NULL.  With only gram asked, no table of size x sites is allocated on the host or copied to it.
 * Accepted and refused as pgbp_sample_posterior_sites, in its order (the reason names pgbp_posterior_cov as the call to use
 * instead where one applies), then: n_cols < 1, c NULL, all three outputs NULL; every refusal before any launch, the outputs,
 * pgbp_layout and the pool untouched.  Scratch is bounded by pgbp_sites_sweep_scratch_limit: chunks are whole workgroups of 256
 * sites (one at least); without gram the columns are cut as the draws of pgbp_sample_posterior_sites are; with gram all n_cols
 * columns of a chunk are resident together, and when the columns of one workgroup of sites -- n_cols size doubles each for w (twice
 * that with k), (blocks + 1) n_cols (n_cols + 1) / 2 for gram and its partial sums, one mark per 64 clusters -- exceed the limit
 * the call is PGBP_ERR_INVALID and the text says how many columns fit.
 * Device: the sampler's validity pass; an ADJOINT phase, one launch per level from the deepest, thread = site, the clusters of the
 * level along grid.y, the columns in a loop, in gather form and in place: a cluster adds to c the terms its children left at
 * their S entries (children in index order, then their S positions in order: pgbp_posterior_cov's list, built once per call;
 * what is taken is left +0.0), forms its at most four coefficients once in registers, and writes w at its R entries and
 * t_C[S_j] = xbar_C[S_j] - sum_i G_ij xbar_C[R_i] at its S entries for its parent -- no factor pool; GRAM, a thread per site and
 * block of 64 entries over all pairs of columns, then the fold; a FORWARD phase, one launch per preorder level, the sampler's
 * apply without its offset and with w for z.  Read-only on the pool, nothing converted.  Two calls return the same bytes, and
 * the bytes of a (column, site) depend neither on the site range nor on the chunks or the other columns.  Values agree with
 * pgbp_posterior_cov to rounding, not to the byte.  EXACT ONLY FOR BELIEFS CALIBRATED ON A CLIQUE TREE; not verified. */
int  pgbp_posterior_cov_sites(pgbp_engine* e, int32_t tree, int32_t site_begin, int32_t site_end, int32_t n_cols,
                              const double* c, double* w, double* k, double* gram, int32_t* info);
/* The same call with the stream drained after each phase (measurement only: tools/time_cov_uni.py): ms5[0 .. 4] = wall
 * milliseconds of {validity pass, adjoint phase, gram and its fold, forward phase, copies of w, k and gram}, summed over the
 * chunks. */
int  pgbp_posterior_cov_sites_timed(pgbp_engine* e, int32_t tree, int32_t site_begin, int32_t site_end, int32_t n_cols,
                                    const double* c, double* w, double* k, double* gram, int32_t* info, double* ms5);
/* IMPUTATION of the missing tip values from CALIBRATED beliefs, for sites [site_begin, site_end): the posterior mean and
 * covariance of the traits a tip does not observe, given ALL the data (the tip's own observed traits included) -- the
 * leave-NOTHING-out complement of pgbp_lg_loo, with the parameters the engine kept from the last pgbp_lg_assignfactors (shared
 * or per site).  EXACT ONLY WHEN THE BELIEFS ARE CALIBRATED (postorder AND preorder) ON A CLIQUE TREE UNDER THOSE PARAMETERS;
 * the call does not verify that.  On a loopy cluster graph, at a converged calibration, it is the Bethe approximation.
 * A family of the table given to pgbp_lg_setup is LISTED when it is a tip family (child_pos < 0, data_row >= 0, n_parents >= 1)
 * whose set M of missing traits (the complement of O = child_mask) is not empty; with NULL masks (complete data) nothing is
 * listed.  Parent k is the FIXED ROOT when parent_pos < 0 and parent_mask is full (its constant qc_k mu enters); any other
 * parent is a CLUSTER parent with scope parent_mask (possibly empty).  The PREDICTED traits are
 *     P = M  intersected with the parent_mask of every cluster parent:
 * a missing trait that some parent does not hold in scope is observed by no tip below that parent, its posterior is in no
 * belief of the graph (it would take a sweep over the ancestors): it is NOT predicted -- NaN in the outputs, visible in the
 * static mask `predicted`.  With Z = O u P, u = sum_k qc_k x_k, w = sum_k wc_k theta, V = sum_k vc_k R[colour_k] (the full
 * p x p matrix; qc, vc, wc as in pgbp_lg_loo), m = J^-1 h and S = J^-1 of the family's cluster:
 *     B = V_PO V_OO^-1 (empty when O is),   mean = E[u_P] + w_P + B (y_O - w_O - E[u_O]),
 *     cov = [-B I] Cov(u_Z) [-B I]' + V_PP - B V_OP,
 *     E[u_T] = sum_k qc_k m[idx_k(T)] (+ qc_k mu_T of the fixed root),  Cov(u_A, u_B) = sum_{a,b} qc_a qc_b S[idx_a(A), idx_b(B)]
 * over the cluster parents, idx_k(t) = parent_pos + popcount(parent_mask below t).  (Given the parents, the tip's noise is
 * independent of every other datum: its observed part is pinned by y_O, the rest is the Gaussian conditional.)
 * pgbp_lg_impute_count: the number n of listed families (-1: no family table); pgbp_lg_impute_families: their indices into
 * the table, in table order -- the order of every output -- and the mask P of each (bit t = trait t); either pointer may be
 * NULL.  Outputs, site-major; either of mean and cov may be NULL, not both:
 *   mean  [sites][n][p]    NaN outside P;
 *   cov   [sites][n][p*p]  column-major, symmetric, both triangles written, NaN in the rows / columns outside P;
 *   info  [sites][n]       (may be NULL) 0; -1: the family's P is empty (all NaN, no solve); 1: V_OO or the conditional variance
 *         V_PP - B V_OP is not positive definite, or the cluster's belief is the constant 1 while a cluster parent is needed;
 *         or 1 + PosDefException.info of the cluster.  Where info is not 0 that (family, site) is all NaN; others are unaffected.
 * Device (csrc/pgbp_impute.hip): one workgroup per (listed family, site) solves the family's cluster in LDS (the solve of
 * pgbp_moments; skipped when no parent is in a cluster) and writes its own p + p*p numbers.  No atomics, no reduction, every
 * sum in index order: two calls return the same bytes, and a site's result does not depend on the other sites of the call.
 * The device copies of the outputs of a chunk of sites at a time (256 MB at most; pgbp_impute_scratch_limit: that bound in
 * doubles, process-wide, <= 0 restores the default -- the results do not depend on the chunks).  Read-only on the beliefs;
 * every layout (a site-minor univariate batch is converted to the plain layout first); one stream synchronisation per call.
 * Fails before any launch, as pgbp_lg_loo: PGBP_ERR_STATE without a family table or before the first pgbp_lg_assignfactors;
 * PGBP_ERR_INVALID for a bad site range, when mean and cov are both NULL, for a family whose cluster has more than 128
 * variables (the family and the cluster are named) or when mom_solve's matrix plus five p x p blocks exceed the 160 KB of
 * LDS -- both taken over the clusters of ALL families of the table, before anything else is decided.
 * A table with nothing listed returns PGBP_OK and writes nothing. */
int32_t pgbp_lg_impute_count(pgbp_engine* e);
int     pgbp_lg_impute_families(pgbp_engine* e, int32_t* fam, uint64_t* predicted);
int     pgbp_lg_impute(pgbp_engine* e, int32_t site_begin, int32_t site_end, double* mean, double* cov, int32_t* info);
void    pgbp_impute_scratch_limit(int64_t doubles);
/* JOINT posterior draws of every cluster variable from CALIBRATED beliefs on a clique tree, for sites [site_begin, site_end):
 * the joint is prod clusters / prod sepsets, and one preorder sweep of schedule tree `tree` (an index into the schedule given to
 * pgbp_set_schedule, as pgbp_traverse's) that conditions each cluster on the sepset to its parent turns standard normals z
 * into exact joint draws x.  The call knows nothing of the evolutionary model: beliefs, scopes and the schedule tree only.
 * Layout: z and x are host pointers, [n_draws][site_end - site_begin][pgbp_sample_size]; cluster i's dims[i] variables sit at
 * the cumulative offset of the cluster dimensions, clusters in index order, variables in the belief's own order
 * (pgbp_sample_size: doubles per (draw, site) = the sum of the cluster dimensions; -1: no engine).
 * Semantics: the parent -> child edges of the tree in its (preorder) order; for the root cluster S is empty; for a child
 * cluster S = the child's variables the sepset to its parent maps to (the child side of that sepset's scope_idx), R = the
 * rest of the child's variables in the child's order; x_S is copied from the parent's already drawn values (read through the
 * parent side of the same scope_idx) and
 *     x_R = J_RR^-1 (h_R - J_RS x_S) + L^-T z_R,     J_RR = L L', L LOWER triangular with a positive diagonal
 * (the Cholesky factor of the R block in the child's variable order; the upper triangle of J is read), z_R = the entries of z
 * at the positions of R: a caller can reproduce a draw from z.  Entries of z at S positions are ignored; a cluster of
 * dimension 0 writes nothing; a sepset of dimension 0 makes the child an independent draw.
 * Consequences: with z = 0 the result is the joint posterior mean; a variable held by several clusters has the same bits in all
 * of them; THE RESULT IS A DRAW FROM THE JOINT POSTERIOR ONLY IF THE BELIEFS ARE CALIBRATED (postorder AND preorder) ON A CLIQUE
 * TREE -- the call does not verify that, as pgbp_lg_gradient does not; the call is read-only on the beliefs and uses no
 * atomics: two calls with the same z return the same bytes; the result for a (draw, site) does not depend on which other draws
 * or sites are in the call.
 * Device (csrc/pgbp_sample.hip): a FACTOR phase, one grid over (cluster, site), eliminates [J_RR | J_RS | h_R] in LDS with the
 * arithmetic of pgbp_moments (at most 16 variables: four clusters per wavefront; 17 .. 64: a wavefront; 65 .. 128: a workgroup
 * of 256 threads) and leaves a = J_RR^-1 h_R, G = J_RR^-1 J_RS and L^-T in a scratch pool no larger than the beliefs, for a chunk
 * of sites at a time (256 MB at most) -- once, however many draws; an APPLY phase, one launch per preorder level over (cluster
 * of the level, draw, variable) x site, x_R = a - G x_S + L^-T z_R with every sum in index order.  z goes up and x comes down
 * as one copy each per chunk, behind one stream synchronisation.  Every layout (a site-minor univariate batch is converted to
 * the plain one first, as pgbp_moments does).
 * Fails before any launch with PGBP_ERR_STATE when no schedule has been set, with PGBP_ERR_INVALID when `tree` is out of range,
 * when the tree does not span every cluster or the graph has a cycle (n_sepsets != n_clusters - 1: the sweep is exact on a
 * clique tree only), for a cluster of more than 128 variables (the message names it, as pgbp_moments'), for n_draws < 1, a bad
 * site range, z or x NULL.
 * info[site - site_begin] (may be NULL): 0, or the 1-based index of the first cluster in preorder whose J_RR is not positive
 * definite: all draws of that site are NaN; other sites are unaffected.  There is no random number generator on the device:
 * the caller supplies z. */
int     pgbp_sample_posterior(pgbp_engine* e, int32_t tree, int32_t site_begin, int32_t site_end, int32_t n_draws,
                              const double* z, double* x, int32_t* info);
int64_t pgbp_sample_size(pgbp_engine* e);
/* Bounds of the scratch of pgbp_sample_posterior, process-wide, in doubles: the factor pool of a chunk of sites (default
 * 32 Mi doubles = 256 MB) and the device copies of z and of x of a chunk of draws (default 128 Mi doubles = 1 GB each); a value
 * <= 0 restores the default.  At least one site and one draw are always taken.  The results do not depend on the chunks (the
 * tests cut a small batch into several to show it). */
void    pgbp_sample_scratch_limits(int64_t factor_doubles, int64_t draw_doubles);
/* The same call with the stream drained after each phase (measurement only: tools/time_sample.py): ms4[0 .. 3] = wall
 * milliseconds of {factor phase, copy of z to the device, apply phase, copy of x to the host}, summed over the chunks. */
int     pgbp_sample_posterior_timed(pgbp_engine* e, int32_t tree, int32_t site_begin, int32_t site_end, int32_t n_draws,
                                    const double* z, double* x, int32_t* info, double* ms4);
/* EXACT posterior covariance between any two entries of the sampler's layout, in the same tree: the adjoint of the sweep above.
 * At one site pgbp_sample_posterior is a linear map x = m + A z, so Cov(x) = A A' and, for a functional c (a weight per entry of
 * the layout), Cov(x, c'x) = A (A'c) and Var(c'x) = |A'c|^2.  `tree`, the site range, size = pgbp_sample_size, the layout of an
 * entry and a cluster's split into S and R are the sampler's.
 *   c [n_cols][size]: the functionals, shared by all sites; a column may put weight on any copy of a variable several clusters hold.
 *   w [n_cols][sites][size] (may be NULL): w = A'c at that site.  Entries at S positions of non-root clusters are +0.0 (the sampler
 *     ignores z there); w_a . w_b = Cov(c_a'x, c_b'x | data).
 *   k [n_cols][sites][size] (may be NULL, not both): k = A w = Cov(x, c'x | data), the covariance of every entry with the functional;
 *     a variable held by several clusters has the same bits in every copy.
 * With T = L^-T (upper triangular) and G = J_RR^-1 J_RS of a cluster, PS the positions of S in the parent:
 *   adjoint, from the deepest level to the root, xbar = c at the start: once all children of C are done
 *     w_C[R_l] = sum_{i <= l} T_il xbar_C[R_i],     xbar_P[PS_j] += xbar_C[S_j] - sum_i G_ij xbar_C[R_i];
 *   forward, from the root: k_C[S_j] = k_P[PS_j],   k_C[R_i] = -sum_j G_ij k_C[S_j] + sum_{l >= i} T_il w_C[R_l].
 * Device (csrc/pgbp_sample.hip): the sampler's FACTOR phase and scratch pool as they are; an ADJOINT phase, one launch per level
 * from the deepest, in gather form -- a thread owns (cluster of the level, column, variable) and adds the terms of the children
 * whose sepsets map to its variable, children in index order, then their S positions in order, from a list the host builds once
 * per call -- and one flat launch for w; a FORWARD phase, one launch per preorder level, the sampler's apply without its offset
 * and with w for z.  No atomics, every sum in a fixed index order: two calls return the same bytes, and the bytes of a (column,
 * site) do not depend on the other columns or sites of the call, nor on the chunks (sites by the factor limit, columns by the
 * draw limit of pgbp_sample_scratch_limits).  Read-only on the beliefs; every layout, as the sampler.  EXACT ONLY FOR BELIEFS
 * CALIBRATED ON A CLIQUE TREE; the call does not verify that.
 * info[site - site_begin] (may be NULL): the sampler's value; w and k of a site whose info is not 0 are NaN, other sites are
 * unaffected.  Fails before any launch as the sampler does, with this function's name in the text: PGBP_ERR_STATE without a
 * schedule; PGBP_ERR_INVALID for `tree` out of range, a tree that does not span or a graph with a cycle, a cluster of more than 128
 * variables, n_cols < 1, a bad site range, c NULL, w and k both NULL. */
int     pgbp_posterior_cov(pgbp_engine* e, int32_t tree, int32_t site_begin, int32_t site_end, int32_t n_cols,
                           const double* c, double* w, double* k, int32_t* info);
/* The same call with the stream drained after each phase (measurement only: tools/time_posterior_cov.py): ms5[0 .. 4] = wall
 * milliseconds of {factor phase, copy of c, adjoint phase with w, forward phase, copies of w and k}, summed over the chunks. */
int     pgbp_posterior_cov_timed(pgbp_engine* e, int32_t tree, int32_t site_begin, int32_t site_end, int32_t n_cols,
                                 const double* c, double* w, double* k, int32_t* info, double* ms5);

/* ---- the model run forwards: simulated traits, and tip data without a new set-up ------------------ */
/* NODE TOPOLOGY of the family table.  pgbp_lg_families names a family's parents by their position in a cluster, which is not
 * enough to walk the network; this call adds who they are:
 *   parent_family [n_families * max_parents]: entry f * K + k = the family whose CHILD is parent k of family f; -1: the fixed
 *                 root (its value is mu); -2: a root without a proper prior (pgbp_lg_simulate is then refused); entries with
 *                 k >= n_parents[f] are not read.
 * Every entry must be in range and < f (families are in preorder: parents come first).  The host levels the table -- the root
 * and a root-prior family have level 0, every other family 1 + the largest level of its parents -- and keeps the families
 * grouped by level on the device.  PGBP_ERR_STATE without a family table; PGBP_ERR_INVALID with NOTHING changed and a text that
 * names the entry ("family F, parent K: ...") otherwise.  A new pgbp_lg_setup clears the topology; pgbp_lg_set_edges,
 * pgbp_lg_set_shifts and pgbp_lg_set_tip_noise leave it alone. */
int     pgbp_lg_set_topology(pgbp_engine* e, const int32_t* parent_family);
/* TIP DATA in and out without a new pgbp_lg_setup, for sites [site_begin, site_end): data [sites][n_rows][p], the set-up's
 * layout.  The missing-data pattern (child_mask) stays the set-up's: an entry outside a tip's mask is stored as the set-up
 * stores it (as given; not finite: 0) and ignored; an entry inside it that is not finite is PGBP_ERR_INVALID with NOTHING
 * changed (the text names the family).  The [row][site] copy of a univariate batch is kept in step.  Takes effect as
 * pgbp_lg_set_shifts does -- at the next pgbp_lg_assignfactors or pgbp_enqueue_loglik_lg; nothing is refilled by the setter --
 * and after that fill the engine's state is bit for bit the state of a fresh engine set up with that data.
 * PGBP_ERR_STATE without a family table, PGBP_ERR_INVALID for a bad site range or a NULL buffer.  One copy (and one transpose
 * launch for a univariate batch) and one stream synchronisation. */
int     pgbp_lg_set_data(pgbp_engine* e, int32_t site_begin, int32_t site_end, const double* data);
int     pgbp_lg_get_data(pgbp_engine* e, int32_t site_begin, int32_t site_end, double* data);
/* SIMULATE every node of the network from the CURRENT model -- the parameters of the last pgbp_lg_assignfactors, the edges,
 * shifts and tip noise in force -- for sites [site_begin, site_end).  Sites are replicates: an engine with B sites yields B data
 * sets (with per-site parameters, shifts or noise each under its own).
 * Semantics.  Families in index order; family f with parents pf(k) = parent_family[f * K + k], the coefficients qc_k, vc_k, wc_k
 * the sweeps use (OU: a = exp(-alpha t), qc = gamma a, vc = gamma^2 (1 - a^2), wc = gamma (1 - a); BM: gamma, gamma^2 t, 0), the
 * shifts s_k and the noise E_f of the site.  The child's state, ALL p traits whatever the scope masks, is
 *     x_f = sum_{k: pf(k) >= 0} qc_k x_pf(k)  +  off_f  +  L_f z_f,
 *     off_f = (sum_k wc_k) theta + sum_k gamma_k s_k + sum_{k: pf(k) = -1} qc_k mu        (the terms in this order),
 *     V_f = sum_k vc_k R[colour_k] (+ E_f) = L_f L_f',   L_f LOWER triangular with a positive diagonal, traits in index order
 * (the lower triangle of V_f is read; (L_f z_f)_t = sum_{j <= t} L_f(t, j) z_f[j] in the order of j).  E_f, all p x p of it, is
 * added for a listed noisy tip: the value is then the OBSERVATION; tips have no children, so the joint law of the tips is the
 * model's.  A root-prior family (no parents) has x = mu + chol(R[colour]) z.  z = 0 gives the prior mean of every node.
 * Layout: z, x and z_out are host pointers, [sites][n_families][p]; x and z_out may be NULL.
 * z == NULL: the device generates the normals itself, from `seed`, and z_out (when not NULL) receives them:
 *     (r0, r1, r2, r3) = Philox4x32-10(counter = (f, t / 2, absolute site, 0), key = (seed & 0xffffffff, seed >> 32))
 *     (Salmon et al. 2011: multipliers 0xD2511F53 on counter word 0 and 0xCD9E8D57 on word 2, key increments 0x9E3779B9 and
 *     0xBB67AE85, ten rounds);
 *     u1 = (((r0 >> 5) << 26 | (r1 >> 6)) + 0.5) * 2^-53,   u2 = the same of (r2, r3)   (doubles; the sum rounded to nearest);
 *     z[t] = sqrt(-2 log u1) cos(2 pi u2) for the even trait t of the pair, z[t + 1] = sqrt(-2 log u1) sin(2 pi u2) for the odd
 *     one (dropped when t + 1 = p), 2 pi = 6.283185307179586.
 * The generator is stateless: the value of a (site, family, trait) does not depend on the site range, on the chunks, or on what
 * else is in the call.  With z != NULL the seed is not read.
 * write_data != 0: every tip family with a data row (child_pos < 0, a data row, a parent edge) writes its child_mask traits into
 * the engine's data (and into the [row][site] copy of a univariate batch) for those sites, as pgbp_lg_set_data would; entries
 * outside the mask keep their bytes; pgbp_lg_get_data then returns exactly x restricted to the tips.  Nothing is refilled.
 * info[site - site_begin] (may be NULL): 0, or the 1-based index of the first family whose V_f is not positive definite: that
 * site's x is NaN and its data are left as they were (with shared parameters, shifts and noise every site then has the same
 * info); other sites are unaffected.
 * Fails before any launch with PGBP_ERR_STATE without a family table, without a topology or before the first
 * pgbp_lg_assignfactors; with PGBP_ERR_INVALID for a -2 parent in the topology (the text names the entry), a bad site range,
 * x and z_out NULL with write_data 0, or p > 64.  Zero-length edges are out of scope, as for the fill.
 * Device (csrc/pgbp_simulate.hip): a FACTOR phase, one grid over (family, parameter set) -- one set when parameters, shifts and
 * noise are all shared (the phase then runs once however many sites), else one per site -- forms V_f in LDS, factors it and
 * leaves [L_f packed | qc | off]; an APPLY phase, one launch per topology level over (family of the level, site, trait).  No
 * atomics, every sum in index order with contraction off: two calls return the same bytes.  Sites are cut into chunks
 * (pgbp_simulate_scratch_limits); with x == NULL the states of a chunk are scratch only.  An engine borrowed from a pgbp_group
 * or pgbp_patterns takes these calls like any other; there is no group-level call. */
int     pgbp_lg_simulate(pgbp_engine* e, int32_t site_begin, int32_t site_end, const double* z, uint64_t seed, double* x,
                         double* z_out, int32_t write_data, int32_t* info);
/* Bounds of the scratch of pgbp_lg_simulate, process-wide, in doubles: the factor records of a chunk of sites (default 32 Mi
 * doubles; one set only when everything is shared) and the states of a chunk, the normals as much again (default 128 Mi
 * doubles each); a value <= 0 restores the default.  At least one site is always taken.  The results do not depend on the
 * chunks. */
void    pgbp_simulate_scratch_limits(int64_t factor_doubles, int64_t state_doubles);
/* The same call with the stream drained after each phase (measurement only: tools/time_simulate.py): ms4[0 .. 3] = wall
 * milliseconds of {factor phase, normals generated or copied up, apply phase, copies to the host}, summed over the chunks. */
int     pgbp_lg_simulate_timed(pgbp_engine* e, int32_t site_begin, int32_t site_end, const double* z, uint64_t seed, double* x,
                               double* z_out, int32_t write_data, int32_t* info, double* ms4);

/* ---- scores (second "next" row: SURVEY.md section 8(f)-2) -------------------------------------- */
/* free_energy(beliefs) (src/score.jl:162-182) for every site: out3[3*site + {0,1,2}] = (average energy,
 * approximate entropy, free energy = energy - entropy); factored_energy (src/score.jl:151-154) = the same
 * with the third value negated (the log-likelihood on a calibrated clique tree).  Uses the factors
 * (ClusterGraphBelief.factor) and the current beliefs.  info[site] (may be NULL) = 0, or 1-based index of the
 * first belief whose precision is not positive definite (its terms are NaN; the reference throws there). */
int  pgbp_free_energy(pgbp_engine* e, double* out3, int32_t* info);

/* ---- factor assignment on the device (first "next" row: SURVEY.md section 8(f)-1) ------------ */
/* assignfactors! (src/beliefs.jl:786-861) for a homogeneous Brownian motion with full rate matrix
 * (MvFullBrownianMotion: factor_treeedge src/evomodels/homogeneousbrownianmotion.jl:262-282,
 * absorbleaf!/absorbevidence! src/beliefupdates.jl:210-274) on a TREE with complete tip data and a fixed
 * root, when every cluster holds at most one node family {child, parent} (clique tree or Bethe graph of a
 * tree).  The static part is given once; every later call only moves the p*p + p + 1 model parameters. */
typedef struct pgbp_bm_tree {
  int32_t p;               /* traits */
  int32_t n_rows;          /* rows of `data` per site */
  const int32_t* kind;     /* [n_clusters] factor of the cluster:
                                0 edge child->parent, both in scope            J = [j -j; -j j], j = R^-1 / t
                                1 edge whose parent is the fixed root          mu absorbed on the parent's variables
                                2 edge whose child is a tip with data          data absorbed on the child's variables
                                3 tip attached to the fixed root               constant
                               -1 no factor (belief = 1), e.g. Bethe variable clusters */
  const double* length;    /* [n_clusters] branch length t > 0 (ignored for kind -1) */
  const int32_t* data_row; /* [n_clusters] row of the tip's data (kinds 2, 3), else -1 */
  const double* data;      /* [n_sites][n_rows][p] tip data, host pointer */
} pgbp_bm_tree;
int  pgbp_bm_tree_setup(pgbp_engine* e, const pgbp_bm_tree* t);
/* Fill every cluster belief AND the factors from (R^-1, log det R, mu), set sepsets to 1, reset the
 * calibration flags: init_beliefs_reset! + the factor loop of assignfactors! + what ClusterGraphBelief /
 * init_messagecalibrationflags_reset! do around it (src/calibration.jl:205-209).
 * Rinv: p*p (column-major, symmetric), mu: p.  per_site != 0: one parameter set per site
 * (Rinv [n_sites][p*p], logdetR [n_sites], mu [n_sites][p]), else one shared set.  Asynchronous. */
int  pgbp_bm_tree_assignfactors(pgbp_engine* e, const double* Rinv, const double* logdetR, const double* mu,
                                int32_t per_site);

/* ---- factor assignment on the device for every linear-Gaussian model of the reference, trees and networks ---- */
/* assignfactors! (src/beliefs.jl:786-861), all parent edges of positive length (no degenerate family); missing tip
 * values through the optional scope masks below (one missingness pattern for all sites of the engine): homogeneous / heterogeneous Brownian motion
 * (src/evomodels/homogeneousbrownianmotion.jl:222-351, heterogeneousmodels.jl:110-150), Ornstein-Uhlenbeck
 * (homogeneousornsteinuhlenbeck.jl:51-66), tree edges (factor_treeedge), hybrid nodes (factor_hybridnode,
 * evomodels.jl:314-330), root prior (factor_root, evomodels.jl:377-396), leaf data and fixed-root mean absorbed
 * (absorbleaf!, absorbevidence!: src/beliefupdates.jl:210-274).  Any cluster graph: a cluster may hold several
 * families (clique trees of networks, join graphs); they are added in the order given, the reference's loop order.
 * Static part (once): one entry per node family that carries a factor, in the order of the reference's loop
 * `for (ni, ci) in enumerate(node2cluster)` (preorder node index); per parent, in the order of node2family[ni][2:end]. */
typedef struct pgbp_lg_families {
  int32_t p;                 /* traits */
  int32_t n_families;
  int32_t max_parents;       /* K >= 1: row length of the per-parent arrays */
  int32_t n_rates;           /* number of p x p variance matrices in pgbp_lg_params.R */
  int32_t n_rows;            /* rows of `data` per site */
  const int32_t* cluster;    /* [n_families] node2cluster[ni] */
  const int32_t* n_parents;  /* [n_families] 0: root prior, 1: tree edge, >= 2: hybrid node */
  const int32_t* child_pos;  /* [n_families] position of the child's first variable in the cluster (its p traits are
                                contiguous: complete data), or -1: a tip, its data row is absorbed */
  const int32_t* data_row;   /* [n_families] row of the tip's data, else -1 */
  const int32_t* parent_pos; /* [n_families * K] position of parent k's first variable, or -1: the fixed root, whose
                                mean is absorbed */
  const double* length;      /* [n_families * K] length of the parent edge, > 0 */
  const double* gamma;       /* [n_families * K] inheritance of the parent edge (1 for a tree edge) */
  const int32_t* color;      /* [n_families * K] index into R of the parent edge's variance rate (heterogeneous models:
                                the edge's colour; homogeneous: 0).  Root prior family: entry [f*K] = index of the
                                prior variance among R */
  const double* data;        /* [n_sites][n_rows][p] tip data, host pointer; entries of traits outside a tip's child_mask
                                are ignored (may be NaN) */
  /* Missing data (both NULL: complete data, every in-scope node has all p traits).  Bit t of a mask = trait t.
   * child_mask[f]: an internal child's traits in scope (inscope column of the cluster belief: src/beliefs.jl:551-559) /
   * a tip's observed traits.  The factor keeps exactly these components of the residual: absorbleaf! marginalises
   * a tip's missing traits (src/beliefupdates.jl:266-274), assignfactors! an internal node's out-of-scope traits
   * (src/beliefs.jl:829-857; valid for the reference's models, whose q is a multiple of the identity).
   * parent_mask[f*K+k]: traits of parent k in scope (its block in the cluster holds popcount of them, in trait order);
   * must contain child_mask[f].  p <= 64. */
  const uint64_t* child_mask;  /* [n_families] or NULL */
  const uint64_t* parent_mask; /* [n_families * K] or NULL */
} pgbp_lg_families;
int  pgbp_lg_setup(pgbp_engine* e, const pgbp_lg_families* f);

enum pgbp_lg_model {
  PGBP_LG_BM = 0,  /* X_child | parents ~ N(sum_k gamma_k X_k, sum_k gamma_k^2 t_k R[color_k]) */
  PGBP_LG_OU = 1   /* a_k = exp(-alpha t_k): N(sum_k gamma_k (a_k X_k + (1 - a_k) theta), sum_k gamma_k^2 (1 - a_k^2) R[color_k]),
                      R = stationary variance sigma2 / (2 alpha); the reference has p = 1 (UnivariateOrnsteinUhlenbeck) */
};
/* Model parameters: everything that changes between two likelihood evaluations.  per_site != 0: one set per site
 * (R [n_sites][n_rates][p*p], alpha [n_sites], theta [n_sites][p], mu [n_sites][p]). */
typedef struct pgbp_lg_params {
  int32_t model;       /* enum pgbp_lg_model */
  int32_t per_site;
  const double* R;     /* [n_rates][p*p] column-major symmetric positive definite */
  const double* alpha; /* OU: [1] */
  const double* theta; /* OU: [p]; NULL for BM */
  const double* mu;    /* [p] root mean (fixed root: the value absorbed; random root: the prior mean) */
} pgbp_lg_params;
/* init_beliefs_reset! + the factor loop of assignfactors! + init_factors_frombeliefs! + flag reset.  A variance
 * sum_k vc_k R[color_k] that is not positive definite (the reference throws) makes that cluster's g NaN.  Asynchronous. */
int  pgbp_lg_assignfactors(pgbp_engine* e, const pgbp_lg_params* m);
/* The whole body of score(theta) (src/calibration.jl:195-221) on the device with the parameters of the LAST
 * pgbp_lg_assignfactors call: factor fill (beliefs only), postorder of tree 0, root integrate. */
int  pgbp_enqueue_loglik_lg(pgbp_engine* e, int32_t reps, const pgbp_opts* opts);

/* ---- device-side access for benchmarking / zero-copy callers ----------------------------- */
/* Enqueue `reps` full calibrate iterations (all trees, post+pre, flag reduction) without any host
 * synchronisation; the caller brackets with pgbp_sync. Resets beliefs from factors before each
 * repetition if reset_each != 0. */
int  pgbp_enqueue_calibrate(pgbp_engine* e, int32_t reps, int32_t reset_each, const pgbp_opts* opts);
/* Enqueue one log-likelihood evaluation body: reset from factors, postorder traversal of tree 0,
 * integrate the root cluster (src/calibration.jl:205-212 minus the host-side factor fill). The
 * per-site norms stay on the device until pgbp_fetch_loglik. */
/* (after an evaluation in which a message of some site failed -- pgbp_fetch_loglik's info[site] != 0 -- the beliefs of THAT
 * site are unspecified, as after a failed traversal of the reference, which stops at once and leaves its beliefs half
 * updated (src/calibration.jl:129-132); in particular the sepsets of that site which the stopped postorder did not reach
 * may still hold an earlier evaluation's values where the engine skipped their reset.  Other sites are unaffected.) */
int  pgbp_enqueue_loglik(pgbp_engine* e, int32_t reps, const pgbp_opts* opts);
int  pgbp_fetch_loglik(pgbp_engine* e, double* norm, int32_t* info);
/* Enqueue integratebelief! of one belief on the CURRENT beliefs (nothing is reset, no message is passed): its per-site
 * constants stay on the device until pgbp_fetch_loglik, like those of pgbp_enqueue_loglik.  No host synchronisation. */
int  pgbp_enqueue_integrate(pgbp_engine* e, int32_t belief);
/* The layout the belief pool is in right now: bit 0 = packed (BS16) records, bit 1 = site-minor univariate batch; 0 = plain.
 * Every call converts as it needs; this only reports (tests of layout independence). */
int32_t pgbp_layout(const pgbp_engine* e);
/* The whole body of score(theta) (src/calibration.jl:195-221) on the device: pgbp_bm_tree_assignfactors with
 * the parameters uploaded by the LAST pgbp_bm_tree_assignfactors call, postorder of tree 0, root integrate. */
int  pgbp_enqueue_loglik_bm(pgbp_engine* e, int32_t reps, const pgbp_opts* opts);
int  pgbp_sync(pgbp_engine* e);
/* The comparison behind the residual-norm flags (iscalibrated_residnorm!, src/beliefs.jl:994-1003): the kernels do not
 * divide, they compare max|dh| (max|dJ|) with the largest x for which fl(x / divisor) <= atol -- divisor = fl(sqrt(s)) for dh,
 * s for dJ.  Pure host function (no device needed): returns that x; +inf for divisor 0 or atol = +inf, -1 (nothing passes)
 * for a NaN or negative atol. */
double pgbp_residual_threshold(double divisor, double atol);
/* Time `reps` repetitions of the enqueued work with HIP events on the engine's stream; returns the
 * total milliseconds in *ms_total and, per kernel family, accumulated device time is NOT measured here
 * (use rocprofv3). kind 0 = calibrate (reset_each honoured), 1 = loglik, 2 = loglik_bm, 3 = loglik_lg (2, 3: with the device factor fill). */
int  pgbp_time_enqueued(pgbp_engine* e, int32_t kind, int32_t reps, int32_t reset_each,
                        const pgbp_opts* opts, float* ms_total);
/* pgbp_enqueue_calibrate with HIP events on the engine's stream around the message launches, so that a caller who times
 * the whole region on the host gets the message kernels' share of exactly those repetitions: with reset_each = 0 ONE
 * event pair around all `reps` repetitions (they run back to back; an event record is a barrier packet, a pair per
 * repetition costs a few percent of a short calibrate), with reset_each != 0 a pair around the message launches of every
 * schedule tree.  pgbp_fetch_kernel_time waits for the stream and returns the sum of the event intervals (*ms_kernels)
 * and the number of message launches inside them. */
int  pgbp_enqueue_calibrate_timed(pgbp_engine* e, int32_t reps, int32_t reset_each, const pgbp_opts* opts);
int  pgbp_fetch_kernel_time(pgbp_engine* e, float* ms_kernels, int32_t* n_launches);
/* Time only the message-kernel launches of `reps` calibrate iterations (reset from factors before each):
 * one HIP event pair on the engine's stream brackets the back-to-back level launches of every traversal;
 * *ms_kernels = sum over traversals, *n_launches = number of level launches inside them. */
int  pgbp_time_message_kernels(pgbp_engine* e, int32_t reps, const pgbp_opts* opts,
                               float* ms_kernels, int32_t* n_launches);
/* Algorithmic bytes of one full calibrate iteration over all sites (SURVEY.md section 8(d) formula:
 * 8*[(mf^2+mf+1) + 4*(s^2+s+1) + (s^2+s)] per message) and message count. */
int  pgbp_traffic_model(const pgbp_engine* e, double* bytes_per_calibrate, int64_t* messages_per_calibrate);

/* ---- several GPUs ---------------------------------------------------------------------------
 * Independent sites are the dimension of the path that shards: calibrate!() of one site never reads another
 * (src/calibration.jl:35-60 works on one ClusterGraphBelief).  One big tree or network on one site does not shard
 * without an exchange step: run replicas (one engine per device).
 *
 * (1) ONE PROCESS, several devices.  A group = one engine (and stream) per listed device over contiguous site ranges
 * (shard i gets sites [first, first + count): the first n_sites % n_devices shards hold one site more).  Every call
 * fans out on one host thread per device and gathers in site order; buffers are the single-engine ones with
 * desc->n_sites = the TOTAL number of sites (desc->device is ignored).  No collective: the host owns every result.
 * A device may be listed more than once (two shards on one GPU: the rehearsal the tests run on a one-GPU box). */
typedef struct pgbp_group pgbp_group;
int  pgbp_group_create(const pgbp_desc* desc, int32_t n_devices, const int32_t* devices, pgbp_group** out);
void pgbp_group_destroy(pgbp_group* g);
const char* pgbp_group_last_error(const pgbp_group* g); /* g == NULL: error of the last failed create (this thread) */
int32_t pgbp_group_size(const pgbp_group* g);
pgbp_engine* pgbp_group_engine(pgbp_group* g, int32_t shard);  /* borrowed: any single-engine call on one shard */
int  pgbp_group_range(const pgbp_group* g, int32_t shard, int32_t* first_site, int32_t* n_sites);
int  pgbp_group_set_schedule(pgbp_group* g, int32_t n_trees, const int32_t* tree_off, const int32_t* pa_j, const int32_t* ch_j);
int  pgbp_group_set_beliefs(pgbp_group* g, const double* packed, int32_t snapshot_factors);
int  pgbp_group_get_beliefs(pgbp_group* g, double* packed);
int  pgbp_group_reset_from_factors(pgbp_group* g);
/* calibrate! on every site; results[n_sites_total].  With auto_stop every site stops at its own first calibrated tree
 * (pgbp_calibrate). */
int  pgbp_group_calibrate(pgbp_group* g, int32_t niter, const pgbp_opts* opts, pgbp_result* results);
int  pgbp_group_integrate(pgbp_group* g, int32_t belief, double* mu, double* norm, int32_t* info);
/* f->data = [n_sites_total][n_rows][p]; per-site parameter sets (m->per_site) = [n_sites_total][...]; each shard takes its
 * rows (n_rates, p: the strides of m->R). */
int  pgbp_group_lg_setup(pgbp_group* g, const pgbp_lg_families* f);
int  pgbp_group_lg_assignfactors(pgbp_group* g, const pgbp_lg_params* m, int32_t n_rates, int32_t p);
int  pgbp_group_enqueue_calibrate(pgbp_group* g, int32_t reps, int32_t reset_each, const pgbp_opts* opts);
int  pgbp_group_enqueue_loglik(pgbp_group* g, int32_t reps, const pgbp_opts* opts);
int  pgbp_group_enqueue_loglik_lg(pgbp_group* g, int32_t reps, const pgbp_opts* opts);
int  pgbp_group_fetch_loglik(pgbp_group* g, double* norm, int32_t* info); /* [n_sites_total] */
int  pgbp_group_sync(pgbp_group* g);

/* ---- several scope patterns behind one handle (src/beliefs.jl:551-559) ------------------------------------------------
 * A site whose data miss other traits at other tips than another site's has other scopes: an internal node has a trait in
 * scope iff some tip below it has a value for it, so belief dimensions and index maps -- the pgbp_desc -- differ.  One
 * engine per PATTERN, the sites that share it batched inside (descs[k]->n_sites of them), on the device descs[k] names;
 * every pattern describes the same cluster graph (clusters, sepsets, their order), so one schedule serves all.
 * sites[sum n_sites]: the caller's (global) index of every site, pattern after pattern: per-site results come back in the
 * caller's order.  Beliefs, factors and family tables have pattern-specific sizes: use pgbp_patterns_engine(k) with the
 * single-engine calls (pgbp_set_beliefs, pgbp_lg_setup, pgbp_lg_assignfactors, ...). */
typedef struct pgbp_patterns pgbp_patterns;
int  pgbp_patterns_create(int32_t n_patterns, const pgbp_desc* const* descs, const int32_t* sites, pgbp_patterns** out);
void pgbp_patterns_destroy(pgbp_patterns* g);
const char* pgbp_patterns_last_error(const pgbp_patterns* g);
int32_t pgbp_patterns_size(const pgbp_patterns* g);
pgbp_engine* pgbp_patterns_engine(pgbp_patterns* g, int32_t pattern);
int  pgbp_patterns_set_schedule(pgbp_patterns* g, int32_t n_trees, const int32_t* tree_off, const int32_t* pa_j,
                                const int32_t* ch_j);
int  pgbp_patterns_calibrate(pgbp_patterns* g, int32_t niter, const pgbp_opts* opts, pgbp_result* results); /* [n_sites] */
int  pgbp_patterns_enqueue_calibrate(pgbp_patterns* g, int32_t reps, int32_t reset_each, const pgbp_opts* opts);
int  pgbp_patterns_enqueue_loglik(pgbp_patterns* g, int32_t reps, const pgbp_opts* opts);
int  pgbp_patterns_enqueue_loglik_lg(pgbp_patterns* g, int32_t reps, const pgbp_opts* opts);
int  pgbp_patterns_fetch_loglik(pgbp_patterns* g, double* norm, int32_t* info);            /* [n_sites], caller's order */
int  pgbp_patterns_integrate(pgbp_patterns* g, int32_t belief, double* norm, int32_t* info); /* [n_sites], caller's order */
int  pgbp_patterns_sync(pgbp_patterns* g);

/* (2) ONE PROCESS PER GPU (torchrun / MPI / Distributed.jl).  Every rank owns an ordinary engine over its own sites;
 * the only exchange is ONE ncclAllGather (RCCL over xGMI) per pgbp_comm_gather_loglik call.  RCCL is bound at run time
 * (dlopen of librccl.so.1, or of the one path in the environment variable PGBP_RCCL_LIB); without it the calls return
 * PGBP_ERR_NO_DEVICE.
 * Rank 0 calls pgbp_comm_unique_id and hands the PGBP_COMM_ID_BYTES to the other ranks by whatever channel launched
 * them; every rank then calls pgbp_comm_create (ncclCommInitRank: collective, blocks until all ranks arrived). */
#define PGBP_COMM_ID_BYTES 128
typedef struct pgbp_comm pgbp_comm;
int  pgbp_comm_unique_id(uint8_t* id /* [PGBP_COMM_ID_BYTES] */);
int  pgbp_comm_create(const uint8_t* id, int32_t n_ranks, int32_t rank, int32_t device, pgbp_comm** out);
void pgbp_comm_destroy(pgbp_comm* c);
const char* pgbp_comm_last_error(const pgbp_comm* c);
/* Every rank contributes, from its engine e (same device as the communicator), the per-site log-likelihoods and info
 * words of its last pgbp_enqueue_loglik* / pgbp_integrate and its sites' (succ, iscal) of the last calibration, in a slot
 * of slot_sites sites (>= the largest number of sites on any rank; the same value on every rank).  On return, on EVERY
 * rank: norm_all[n_ranks * slot_sites] and info_all (may be NULL) hold rank r's sites at [r * slot_sites, ...) (unused
 * tail of a slot: 0), *all_succ / *all_iscal (may be NULL) the minimum over all sites of all ranks -- the
 * all-reduce(min) of the flags SURVEY.md section 8(e) asks for, carried by the same collective.  Enqueued on the engine's
 * stream behind the kernels that produce the values; returns after the result reached the host. */
int  pgbp_comm_gather_loglik(pgbp_comm* c, pgbp_engine* e, int32_t slot_sites, double* norm_all, int32_t* info_all,
                             int32_t* all_succ, int32_t* all_iscal);
/* What can fail on THIS rank before the collective pgbp_comm_create (RCCL not loadable, no such device), without
 * touching the other ranks: a launcher takes the minimum of (status == 0) over its ranks and only then lets every rank
 * enter pgbp_comm_create -- a rank that fails there alone would leave its peers blocked inside ncclCommInitRank. */
int  pgbp_comm_precheck(int32_t device);
/* The exchange step of a cluster graph CUT across ranks (the loop of src/calibration.jl:46-47 with each traversal,
 * src/calibration.jl:111-161, cut by spanning-tree subtrees: DESIGN.md section 6): rank r contributes the records (J, h, g;
 * the packing of pgbp_get_belief) of the beliefs lists[list_off[r] .. list_off[r + 1]) of `site`; ONE ncclAllGather carries
 * them, and every rank overwrites its copies of the other ranks' beliefs.  Every rank passes the same lists (the cut is a
 * function of the schedule).  Device to device: the payload never visits the host.  include_self != 0: a rank also
 * overwrites its own listed beliefs from its own slot (a self-test of the path on one rank). */
int  pgbp_comm_exchange_beliefs(pgbp_comm* c, pgbp_engine* e, int32_t site, const int32_t* list_off, const int32_t* lists,
                                int32_t include_self);
/* The host-side half of pgbp_comm_gather_loglik on its own (no GPU, no RCCL): recv = the gathered buffer, n_ranks slots
 * of 2 * slot_sites + 2 doubles each, a slot = [norm (slot_sites) | info (slot_sites) | succ | iscal] as a rank packs it;
 * outputs as for pgbp_comm_gather_loglik. */
int  pgbp_comm_unpack_slots(const double* recv, int32_t n_ranks, int32_t slot_sites, double* norm_all, int32_t* info_all,
                            int32_t* all_succ, int32_t* all_iscal);

#ifdef __cplusplus
}
#endif
#endif /* PGBP_H */
