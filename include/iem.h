/* iem.h — C-ABI of libiem_hip.so: the MI355X evaluation backend for
 * InfiniteOpt → ExaModels transcriptions.
 *
 * The reference reaches its evaluator through Julia method calls on an
 * ExaModels.ExaModel built at /root/reference/src/infiniteopt_backend.jl:155-156
 * (`ExaModels.ExaCore(model, data; backend)` → `ExaModels.ExaModel(core)`); the NLP
 * solvers then call the NLPModels API on it every iteration
 * (/root/reference/ext/InfiniteExaModelsIpopt.jl:48-49,59-60,
 *  /root/reference/ext/InfiniteExaModelsMadNLP.jl:49-50,64).  Each entry point
 * below replaces one of those calls; a Julia `ccall` / Python `ctypes` shim binds
 * them one to one.
 *
 * Conventions
 *   - every function returns 0 on success, a negative IEM_E_* code otherwise; the
 *     message is in iem_last_error() (thread-local).  Nothing throws across the ABI.
 *   - `d_` arguments are DEVICE pointers (ROCArray / torch data_ptr), `h_` are HOST
 *     pointers.  The caller owns every array; outputs are fully overwritten.
 *   - evaluation calls are enqueued on the handle's stream and return immediately,
 *     except iem_obj (returns a host scalar) and the *_structure calls.
 *   - a handle is not thread-safe; use one per solver.
 */
#ifndef IEM_H
#define IEM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct iem_model iem_model;

enum {
  IEM_OK = 0,
  IEM_E_BLOB = -1,    /* malformed / unsupported blob                     */
  IEM_E_HIP = -2,     /* HIP runtime error                                */
  IEM_E_COMPILE = -3, /* kernel generation / hiprtc failure               */
  IEM_E_ARG = -4,     /* bad argument                                     */
  IEM_E_NODEVICE = -5,/* no usable gfx950 device                          */
  IEM_E_COMM = -6     /* a mailbox wait (halo exchange / fold / all-reduce) timed out since the last check: a peer did not take
                         part.  The kernels have set what they should have delivered to NaN; reported once, by the next host
                         synchronisation point (iem_obj, iem_obj_end, iem_synchronize), then cleared                         */
};

/* mirrors NLPModels' `meta` fields the reference reads
 * (infiniteopt_backend.jl:600-601 get_x0/get_y0; ext/InfiniteExaModels{Ipopt,MadNLP}.jl solver construction) */
typedef struct iem_meta_t {
  int64_t nvar, ncon, npar;
  int64_t nnzj, nnzh;
  int64_t n_templates;
  int32_t minimize;
  int32_t n_kernels; /* fused kernels generated for this model */
} iem_meta_t;

/* which host mirror iem_get_host returns */
enum { IEM_X0 = 0, IEM_LVAR = 1, IEM_UVAR = 2, IEM_LCON = 3, IEM_UCON = 4, IEM_Y0 = 5, IEM_THETA = 6 };

/* per-template layout (ExaModels SIMDFunction offsets o0/o1/o2 and steps) */
typedef struct iem_template_info_t {
  int64_t kind; /* 0 objective, 1 constraint */
  int64_t n_items, o0, o1, o2, o1step, o2step;
} iem_template_info_t;

/* one fused kernel of the model: launch shape and ALGORITHMIC traffic (every distinct
 * input element read once, every output element written once) — what the roofline
 * line of bench.py is computed from */
typedef struct iem_kernel_info_t {
  char name[64];
  int32_t kind; /* 0 cons, 1 jac, 2 hess, 3 obj, 4 grad, 5 jprod, 6 jtprod, 7 hprod, 8 jac + hess in one launch (iem_jac_hess_coord) */
  int32_t jit;  /* 1 if this model's code object was compiled by hiprtc (cache miss) */
  int64_t grid[3];
  int64_t lds_bytes;
  int64_t alg_bytes_read, alg_bytes_written;
} iem_kernel_info_t;

/* ---- lifecycle -----------------------------------------------------------
 * iem_create   replaces ExaModels.ExaModel(core) with backend = MI355XBackend()
 *              (infiniteopt_backend.jl:155-156; README.md:41 `backend = CUDABackend()`).
 *              `blob` is the transcribed model (include/iem_blob.h). */
int iem_create(const void *blob, size_t nbytes, int device, iem_model **out);
/* The same with per-HANDLE generator options: the process-wide defaults (iem_set_option) with
 * `opts[0 .. n_opts)` applied on top, for this model only — two models with different layouts
 * (e.g. a merged-Hessian one next to a default one) coexist in one process.  Option names as for
 * iem_set_option. */
typedef struct iem_option_t {
  const char *name;
  int64_t value;
} iem_option_t;
int iem_create_opts(const void *blob, size_t nbytes, int device, const iem_option_t *opts, int n_opts, iem_model **out);

/* ---- multi-GPU: one process (or one handle) per GPU ------------------------------------------
 * The reference is single-device; its templates are embarrassingly parallel over the supports of
 * an infinite parameter, so the path shards by support: rank r of `world` owns a
 * contiguous block of the supports of parameter group `group` (the 1-based group id the blob's grid
 * hints and slab table use: 1 = the first infinite parameter).  iem_create_sharded takes the GLOBAL
 * blob — exactly what iem_create takes — and cuts the rank's window in C++ (csrc/iem_shard.hpp): local
 * x = window slices of the sharded slabs (with the stencil's halo in front: 1 support for backward
 * differences, the element's first support for orthogonal collocation) + replicated slabs; templates over
 * the group are cut to the owned supports (whole elements for collocation boxes, filtered lists for domain
 * restrictions); cons!/jac_coord!/hess_coord! then need no communication at all.  Two exchanges remain:
 *   iem_halo_exchange        before cons!/jac!/hess!: the stencil neighbours  x_k[a_r - 1]
 *                            (transform.jl:535-557) from the left rank into the halo entries of x
 *   iem_allreduce_obj_grad   after obj / grad!: the scalar objective and the gradient entries of
 *                            replicated variables, summed over ranks in rank order (bitwise equal
 *                            on every rank)
 *   (iem_halo_fold           the transpose of the first, for J'v / Hv on a rank's rows)
 * Each is one small kernel that writes straight into the peers' mailboxes (HIP IPC; xGMI between
 * GPUs) and waits on its own — asynchronous on the handle's stream, graph-replayable, every wait
 * bounded (iem_comm_status reports a time-out).  Wiring: every rank calls iem_comm_export, the host
 * all-gathers the IEM_COMM_HANDLE_BYTES-byte handles (MPI / torch.distributed / a pipe — like an
 * ncclUniqueId), every rank calls iem_comm_connect with all of them in rank order. */
typedef struct iem_shard_t {
  int32_t group, rank, world;
  int32_t mailbox_kind;        /* 0 no mailbox yet; 1 uncached, 3 fine-grained device memory (coherent across GPUs); 2 plain hipMalloc (one-GPU rehearsal only) */
  int64_t n_global;            /* supports of the sharded group                       */
  int64_t own_lo, own_n, halo; /* first owned support (global, 0-based), count, halo supports in front */
  int64_t halo_reach, halo_doubles;
  int64_t nvar_global, ncon_global, nnzj_global, nnzh_global;
  int64_t nvar, ncon, nnzj, nnzh, n_templates; /* this rank's shard */
  int64_t n_shared;            /* replicated variables = gradient entries the all-reduce sums */
} iem_shard_t;
/* a local template and where its items sit in the global model: local item coordinate k_d = global
 * coordinate klo[d] + k_d of the box global_dims; global COO position of local slot s of item k:
 * global_o1 + o1step * (global ordinal of k) + s  (likewise o2; rows: global_o0 + ordinal) */
typedef struct iem_shard_template_t {
  int64_t global_index, kind, n_items;
  int64_t klo[3], dims[3], global_dims[3];
  int64_t o0, o1, o2, global_o0, global_o1, global_o2;
  int64_t o1step, o2step;
  /* -1: the local items are the box klo .. klo + dims of global_dims; >= 0: the template is an explicit item
   * list (a domain restriction filtered its iterator, transform.jl:448-451) and local item j is global item
   * items[items_offset + j] of the array iem_shard_template_items / iem_shard_blob hand out */
  int64_t items_offset;
} iem_shard_template_t;
#define IEM_COMM_HANDLE_BYTES 128
int iem_create_sharded(const void *blob, size_t nbytes, int device, int group, int rank, int world,
                       const iem_option_t *opts, int n_opts, iem_model **out);
int iem_shard_info(const iem_model *m, iem_shard_t *out);
/* local variable -> global variable (0-based), and per local variable: bit 0 owned by this rank,
 * bit 1 replicated on every rank, bit 2 halo copy of the LEFT neighbour's variable (in front of the owned block),
 * bit 3 halo copy of the RIGHT neighbour's variable (behind it: forward / central differences) (either may be NULL) */
int iem_shard_var_map(const iem_model *m, int64_t *h_map, uint8_t *h_flag);
/* Both directions of the halo (iem_shard_t keeps its layout: its halo / halo_reach / halo_doubles are the FRONT halo):
 * out = {halo_left, halo_right, reach_left, reach_right, doubles_to_right, doubles_to_left} — the halo supports this rank
 * carries in front of / behind its owned block, the model's stencil reach to the left / right (backward differences:
 * 1 / 0, forward: 0 / 1, central: 1 / 1; transform.jl:535), and the doubles one rank sends its right / left neighbour
 * per exchange.  A shard with reach_right > 0 exchanges (and folds) both ways in ONE kernel: all sends before all waits. */
int iem_shard_halo(const iem_model *m, int64_t out[6]);
int iem_shard_template_info(const iem_model *m, int64_t i, iem_shard_template_t *out);
/* global item ordinals of every explicit-list template, concatenated (see items_offset); h_items may be NULL to
 * query the length */
int iem_shard_template_items(const iem_model *m, int64_t *h_items, int64_t *out_n);
/* the cut without a device (tooling / tests): the rank's shard re-serialised as a blob of its own, plus
 * the maps; every out array is malloc'ed (iem_free), any of the last five may be NULL */
int iem_shard_blob(const void *blob, size_t nbytes, int group, int rank, int world, void **out_blob, size_t *out_nbytes,
                   iem_shard_t *out_info, int64_t **out_var_map, uint8_t **out_var_flag, iem_shard_template_t **out_tpl,
                   int64_t **out_items);
int iem_comm_export(iem_model *m, void *out_handle /* IEM_COMM_HANDLE_BYTES */);
int iem_comm_connect(iem_model *m, const void *all_handles /* world x IEM_COMM_HANDLE_BYTES, rank order */);
int iem_halo_exchange(iem_model *m, double *d_x);
/* The same exchange OFF the critical path — nothing is launched for it.  The call only DEFERS the exchange; it then rides on
 * the first evaluation launch that takes the same d_x and whose kernels cannot touch a halo entry of it: ONE EXTRA LEADING
 * WORKGROUP of that kernel sends my boundary supports to the right neighbour, waits (bounded) for the left neighbour's,
 * writes them into the halo entries of d_x and acknowledges, while the kernel's other workgroups evaluate — no launch, no
 * stream, no event of its own, and every kernel launched BEHIND that one sees the halo entries as after iem_halo_exchange.
 * Which calls can carry it follows from what their generated kernels load (iem_halo_reads): obj, and jac_coord! /
 * hess_coord! / iem_jac_hess_coord whenever the stencil rows are linear (their partials are item data — the reference's
 * derivative approximations, transform.jl:511-562); cons! of such a model reads x_k[a_r - 1] (transform.jl:535-557): if it
 * comes first, it gets the stand-alone exchange kernel in front of it — exactly iem_halo_exchange.  In solver order (obj,
 * grad!, cons!, jac_coord!, hess_coord! at a new point: ext/InfiniteExaModelsIpopt.jl:48-49) the exchange rides on obj and is
 * complete before cons! starts.  A call that neither touches nor can carry (grad!, the products) leaves it deferred;
 * iem_halo_wait, iem_synchronize, iem_halo_fold, iem_allreduce_obj_grad, iem_comm_status and a further exchange flush it
 * (stand-alone kernel).  ORDERING RULE: every rank issues its mailbox kernels in the same order — whether an evaluation
 * call carries or flushes a deferred exchange depends on the rank's own halo (rank 0 has none), so no collective
 * (fold, all-reduce) ever overtakes a deferred exchange: each flushes it first.
 * Contract: between this call and the evaluation call that carries it (or iem_halo_wait) the caller enqueues nothing that
 * writes d_x or reads its halo entries.  Graph-capturable (the decision is taken at capture time; a replay repeats it).
 * iem_halo_reads: for kernel kind `kind` (iem_kernel_info_t.kind): can it touch a halo entry through x / through a
 * variable-space v, and can it carry a deferred exchange of x. */
int iem_halo_exchange_async(iem_model *m, double *d_x);
int iem_halo_wait(iem_model *m);
int iem_halo_reads(const iem_model *m, int kind, int *out_x, int *out_v, int *out_carrier);
/* The transposed exchange, for a vector in VARIABLE space produced by a transposed operator on this rank's rows
 * (iem_jtprod): the entries of the halo copies hold what this rank's rows owe to variables the LEFT neighbour owns
 * (the x_k[a_r - 1] column of the first difference row, src/transform.jl:535-557).  They are sent to the left
 * neighbour, which ADDS them to its owned entries (one addend per entry: order-independent), and zeroed here.
 * A two-sided shard (iem_shard_halo: reach_right > 0) also sends its BACK halo copies to the right neighbour; an owned
 * entry then takes the left neighbour's addend first, the right neighbour's second — a fixed order, reproducible bits.
 * Entries of replicated variables are summed with iem_allreduce_obj_grad (d_obj may be NULL).  Asynchronous on the
 * handle's stream, graph-capturable, bounded waits like iem_halo_exchange. */
int iem_halo_fold(iem_model *m, double *d_vec);
int iem_allreduce_obj_grad(iem_model *m, double *d_obj /* device scalar, may be NULL */, double *d_g);
/* synchronises the handle's stream; 0 = every exchange so far completed, else a bit mask of time-outs (1 / 2 halo ack / data,
 * 4 all-reduce, 8 / 16 fold ack / data; the second direction of a two-way exchange: 32 / 64 halo ack / data, 128 / 256 fold
 * ack / data).  A time-out never hangs and never goes unnoticed: the kernel that ran into it writes
 * NaN instead of the data that did not arrive, and the next iem_obj / iem_obj_end / iem_synchronize returns IEM_E_COMM (and
 * clears the mask).  The bound is the per-handle option "comm_timeout_ms" (default 5000). */
int iem_comm_status(iem_model *m, int64_t *out_status);

int iem_destroy(iem_model *m);
int iem_meta(const iem_model *m, iem_meta_t *out);
int iem_template_info(const iem_model *m, int64_t i, iem_template_info_t *out);
int iem_kernel_info(const iem_model *m, int k, iem_kernel_info_t *out);
int iem_get_host(const iem_model *m, int which, double *h_out);
int iem_set_stream(iem_model *m, void *hip_stream);
int iem_synchronize(iem_model *m);

/* ExaModels.set_parameter!(core, param, vals)  (infiniteopt_backend.jl:522-526,546):
 * overwrite θ[off .. off+len) (0-based offset) from a host array. */
int iem_set_parameter(iem_model *m, int64_t off, int64_t len, const double *h_vals);

/* ---- NLPModels evaluation API ------------------------------------------------
 * obj / grad! / cons! / jac_coord! / hess_coord!(m, x, y, vals; obj_weight) as called by
 * the solvers (ext/InfiniteExaModelsIpopt.jl:49, ext/InfiniteExaModelsMadNLP.jl:50). */
int iem_obj(iem_model *m, const double *d_x, double *h_out);
int iem_obj_device(iem_model *m, const double *d_x, double *d_out); /* async variant */
/* iem_obj in two halves: begin enqueues the objective kernel (its last workgroup writes the scalar into mapped host memory) and
 * returns at once, end waits for the value.  A solver that evaluates obj, grad!, cons!, jac_coord!, hess_coord! at one point
 * (ext/InfiniteExaModelsIpopt.jl:48-49) calls begin first and end after its last launch: the host round trip of the scalar
 * (~8 us of the ~14 us iem_obj takes on a small model) overlaps the other four calls.  One begin outstanding per handle. */
int iem_obj_begin(iem_model *m, const double *d_x);
int iem_obj_end(iem_model *m, double *h_out);
int iem_grad(iem_model *m, const double *d_x, double *d_g);
int iem_cons(iem_model *m, const double *d_x, double *d_c);
int iem_jac_coord(iem_model *m, const double *d_x, double *d_vals);
int iem_hess_coord(iem_model *m, const double *d_x, const double *d_y, double obj_weight, double *d_vals);
/* jac_coord!(m, x, jac) + hess_coord!(m, x, y, hess; obj_weight) in ONE launch: the two are independent given x and y
 * (MadNLP evaluates both at every accepted point, ext/InfiniteExaModelsMadNLP.jl:49-50,64).  Identical bytes to the two
 * calls; one launch ramp and drain instead of two, and on a shard-sized grid (about one workgroup per CU and kind) both
 * kinds are resident together. */
int iem_jac_hess_coord(iem_model *m, const double *d_x, const double *d_y, double obj_weight, double *d_jac, double *d_hess);

/* One launch per SOLVER PHASE (extensions; identical bytes to the separate calls, which remain).  An interior-point solver
 * evaluates obj + cons! at every trial point of its line search and grad! + jac_coord! + hess_coord! once per accepted
 * point (ext/InfiniteExaModelsMadNLP.jl:49-50,64, ext/InfiniteExaModelsIpopt.jl:48-49 of the reference); on the grids
 * the reference benchmarks (ESCAPE34/run_cases_gpu.jl:89-102: 1 000 - 16 000 supports) every call is one 5-7 us launch,
 * so the phase costs what its launches cost.
 *   iem_eval_trial     c = cons(x) into d_c and f = obj(x): returned in *h_obj (the call then waits for the scalar, like
 *                      iem_obj), or — h_obj == NULL — collected later by iem_obj_end (the call arms it like iem_obj_begin)
 *   iem_eval_accepted  g = grad(x), jac values, Lagrangian Hessian values (obj_weight, y) — asynchronous on the stream
 * Outputs are fully overwritten.  Handles without the fused kernels make the separate calls themselves. */
int iem_eval_trial(iem_model *m, const double *d_x, double *d_c, double *h_obj /* may be NULL */);
int iem_eval_accepted(iem_model *m, const double *d_x, const double *d_y, double obj_weight, double *d_g, double *d_jac, double *d_hess);
/* ... and all five of ONE point in one launch — the solver's first trial point is usually the accepted one; h_obj as above */
int iem_eval_all(iem_model *m, const double *d_x, const double *d_y, double obj_weight, double *d_c, double *d_g, double *d_jac, double *d_hess,
                 double *h_obj /* may be NULL */);

/* The CONVERGENCE CHECK of a solver (extensions): the dual residual  obj_weight*grad f(x) + J(x)' y  — the gradient of the
 * Lagrangian; the dual infeasibility of Ipopt / MadNLP is this vector minus the bound multipliers — from ONE kernel, and
 * with c(x) and f(x) from ONE launch:
 *   iem_lagrad         out = obj_weight*grad f(x) + J(x)' y        y: ncon, out: nvar
 *   iem_eval_residual  the same vector into d_lagrad, c = cons(x) into d_c, f = obj(x) into the DEVICE scalar d_obj
 *                      (as iem_obj_device: no mapped host slot, nothing to collect with iem_obj_end)
 * In the kernel an objective template is seeded with obj_weight and a constraint template with y[row] (as iem_jptprod does
 * for θ), every first-order slot is kept, and ONE deterministic scatter handles both: no float atomics, bitwise reproducible
 * from call to call; entries of x no template touches get 0, the outputs are fully overwritten.  d_lagrad is bitwise what
 * iem_lagrad writes, d_c what iem_cons writes, d_obj what iem_obj_device writes.  ncon == 0: d_y and d_c may be NULL and the
 * vector is obj_weight*grad f; a model without objective gets d_obj = 0; a model without any first-order slot: a memset.
 * The kernels (kinds 0 / 3 / 6 — names iem_cons*, iem_obj*, iem_lagrad* — and the phase kernel iem_residual_all, kind 9) are
 * a SIXTH program of their own over the plain model, set up by the first of the two calls — synchronous, outside a stream
 * capture; every later call is asynchronous on the handle's stream and capturable — or by iem_lagrad_prepare (idempotent;
 * returns the number of this program's kernels; a runtime failure of the set-up is not remembered).  The other prepare
 * calls do not prepare it and keep their counts; iem_kernel_info lists these kernels behind those of the θ programs, in the
 * full order  model / three kinds / adjoint / θθ / θ-COO / residual / scaled  (every program that exists on the handle;
 * only the scaled program's kernels come behind these), with their algorithmic bytes — the phase kernel reports the union
 * of its members' reads.  Where the phase kernel does not exist (a member missing, kinds of different workgroup sizes, more
 * workgroups than one launch takes) iem_eval_residual makes the member launches itself.  A sharded handle refuses all three
 * calls with IEM_E_ARG: the result would need the halo fold and the all-reduce. */
int iem_lagrad_prepare(iem_model *m, int32_t *out_n_kernels);
int iem_lagrad(iem_model *m, const double *d_x, const double *d_y, double obj_weight, double *d_out /* nvar */);
int iem_eval_residual(iem_model *m, const double *d_x, const double *d_y, double obj_weight,
                      double *d_c /* ncon */, double *d_lagrad /* nvar */, double *d_obj /* device scalar */);

/* ROW SCALING inside the kernels (extensions): what a solver that scales the NLP — Ipopt's gradient-based scaling, MadNLP's
 * scale_constraints! — does around jac_coord! and cons!, without a pass over nnzj of its own:
 *   iem_jac_rowmax        out[r] = max over the first-order slots of row r of |dc_r/dx_slot| — the COO entries iem_jac_coord
 *                         writes with row r; repeated positions are NOT summed (the solvers take the maximum over the
 *                         triplets); EVERY row is written, 0.0 for a row without a slot; a NaN slot gives NaN for its row
 *   iem_cons_scaled       out[r] = s[r] * c_r(x)
 *   iem_jac_coord_scaled  out[k] = s[row(k)] * jac[k], at the positions of iem_jac_structure
 * Under the default options (fp_contract = 0), on one handle at one (x, θ): iem_cons_scaled is bitwise fl(s * c) of what
 * iem_cons writes, iem_jac_coord_scaled bitwise fl(s[row] * v) of what iem_jac_coord writes — ONE rounded multiply of the
 * finished value, data rows and computed rows alike — and iem_jac_rowmax bitwise the per-row maximum of |.| over what
 * iem_jac_coord writes.  The objective and the Hessian need nothing new: iem_hess_coord(x, y .* s, obj_weight * s_f) is the
 * scaled Hessian.  One lane per item, an item is one row: the maximum is a per-lane reduction with one exclusive store per
 * row, the scaling one load of s[row] per row and a multiply per slot in front of the store path of jac_coord! / cons!; no
 * atomics, every entry stored once, outputs fully overwritten, the handle's current θ (iem_set_parameter) is seen.
 * The kernels (kinds 5 / 0 / 1, names iem_rowmax*, iem_cons_scaled*, iem_jac_scaled*) are a SEVENTH program of their own
 * over the plain model, set up by the first of the three calls — synchronous, outside a stream capture; every later call is
 * asynchronous on the handle's stream and capturable — or by iem_scaled_prepare (idempotent; returns the number of this
 * program's kernels; a runtime failure of the set-up is not remembered).  The other prepare calls do not prepare it and
 * keep their counts; iem_kernel_info lists these kernels LAST: model / three kinds / adjoint / θθ / θ-COO / residual /
 * scaled, with their algorithmic bytes.  ncon == 0 or nnzj == 0: nothing is launched for the empty output, NULL is accepted
 * for a zero-length array.  A sharded handle refuses all four calls with IEM_E_ARG: the values need no communication, but
 * the deferred halo exchange (carrier workgroup, flush logic) is not taught this program — out of scope. */
int iem_scaled_prepare(iem_model *m, int32_t *out_n_kernels);
int iem_jac_rowmax(iem_model *m, const double *d_x, double *d_rowmax /* ncon */);
int iem_cons_scaled(iem_model *m, const double *d_x, const double *d_s /* ncon */, double *d_c /* ncon */);
int iem_jac_coord_scaled(iem_model *m, const double *d_x, const double *d_s /* ncon */, double *d_vals /* nnzj */);

/* ---- the KKT operator in one launch ------------------------------------------------------------------------------------------
 * out_x = W u + J' v,  out_y = J u   with  W = obj_weight ∇²f(x) + Σ_r y_r ∇²c_r(x)  (the full symmetric operator, as iem_hprod
 * applies it) and J = ∂c/∂x: the product with K0 = [W, J'; J, 0] that a Newton step's residual and every matrix-free method need,
 * from ONE launch (kernel iem_kktprod_all: the x-part is hprod's symbolic sweep with one more addend per first-order slot of a
 * constraint row, v[row] ∂c_row/∂x_slot, through one deterministic scatter — no float atomic, bitwise reproducible; the y-part
 * is the model's own jprod body, out_y carries the bits of iem_jprod).  Where that kernel does not exist (no constraint, kinds
 * of different workgroup sizes, more workgroups than one launch takes) the two member launches are made.  An entry of out_x no
 * template touches is 0; both outputs are fully overwritten; the handle's current θ is seen.  d_v == NULL means v = 0
 * (out_x = W u).  ncon == 0: d_y, d_v and d_out_y may be NULL.  The outputs may not overlap each other or an input: IEM_E_ARG.
 * The kernels (kinds 7 / 5 / 9, names iem_kktx*, iem_kkty*, iem_kktprod_all) are an EIGHTH program of their own over the plain
 * model, set up by the first call — synchronous, outside a stream capture; every later call is asynchronous on the handle's
 * stream and capturable — or by iem_kktprod_prepare (idempotent; the number of this program's kernels).  The other prepare
 * calls do not prepare it and keep their counts; iem_kernel_info lists these kernels LAST, behind the scaled program's.
 * A sharded handle refuses both calls with IEM_E_ARG (the x-part would need the halo fold of hprod and jtprod). */
int iem_kktprod_prepare(iem_model *m, int32_t *out_n_kernels);
int iem_kktprod(iem_model *m, const double *d_x, const double *d_y, double obj_weight, const double *d_u /* nvar */,
                const double *d_v /* ncon, NULL = 0 */, double *d_out_x /* nvar */, double *d_out_y /* ncon */);

/* ---- one launch per solver phase for the SCALED NLP ---------------------------------------------------------------------------
 * A solver that scales its NLP (s = d_s: ncon row factors, obj_scale = s_f) evaluates, per trial point, s∘c(x) and s_f·f(x),
 * and per accepted point s_f·∇f(x), the row-scaled Jacobian and the Hessian of  σ·s_f·f + (y∘s)'c:
 *   iem_eval_trial_scaled     c = iem_cons_scaled(x, s) and *h_obj = obj_scale * iem_obj(x), ONE launch (iem_sp_trial_all)
 *   iem_eval_accepted_scaled  g = iem_grad_scaled(x, obj_scale), jac = iem_jac_coord_scaled(x, s) and
 *                             hess = iem_hess_coord_scaled(x, y, s, fl(obj_weight * obj_scale)), ONE launch
 *                             (iem_sp_accepted_all) and sp_grad's follow-ups; the product of the two scalars is formed
 *                             here, in host double arithmetic
 *   iem_grad_scaled           obj_scale * ∇f(x): grad!'s reverse sweep seeded with obj_scale instead of 1.0
 *   iem_hess_coord_scaled     iem_hess_coord(x, fl(y∘s), obj_weight): a constraint row's multiplier is ONE rounded multiply
 *                             y[row] * s[row] in the kernel; obj_weight is the weight AS USED (the caller has multiplied in s_f)
 * Under the default options (fp_contract = 0), on one handle at one (x, θ): c, jac and hess carry the bits of the calls named
 * above (hess: of iem_hess_coord with y∘s formed by one float64 multiply per row), *h_obj is bitwise obj_scale * iem_obj(x),
 * the phases' outputs carry the bits of the member calls.  iem_grad_scaled(x, 1.0) and (x, 2^k) equal iem_grad(x) and
 * 2^k * iem_grad(x) as IEEE values (NaNs in the same places; the sign of a zero may differ, a folded 0.0 + v against a
 * runtime one); a general factor agrees to rounding.  No float atomic in any kernel: every call is bitwise reproducible.
 * The objective: the kernel writes the model's own f into the mapped host slot, exactly as iem_eval_trial arms and collects
 * it, and the library returns obj_scale * f.  With h_obj == NULL the handle remembers the factor and iem_obj_end applies it
 * to THAT pending value; every later arm (iem_obj_begin, iem_eval_trial, iem_eval_all, this call) resets it, a pending
 * unscaled value is returned untouched.  The deferred form (h_obj == NULL ... iem_obj_end) must NOT be captured in a graph:
 * the sentinel is armed and the slot read on the host; the call with h_obj waits on the host and cannot be captured either.
 * Where a phase kernel does not exist (option "phase_kernels" = 0, a member missing — no objective, no constraint —, more
 * workgroups than one launch takes) the member launches are made.  ncon == 0: d_s, d_y, d_c and d_jac may be NULL; a model
 * without an objective gives g = 0 (the runtime's memsets) and f = 0; a linear program has no Hessian member.
 * The kernels (kinds 0 / 1 / 2 / 3 / 4 / 9 / 10, names iem_sp_cons*, iem_sp_jac*, iem_sp_hess*, iem_sp_obj*, iem_sp_grad*,
 * iem_sp_trial_all, iem_sp_accepted_all) are a NINTH program of their own over the plain model — the model's tile on every
 * grid, its own reduction buffer, axis sums and gather plan for the gradient —, set up by the first of the four calls —
 * synchronous, outside a stream capture; every later call is asynchronous on the handle's stream and capturable, except
 * for the host-collected objective — or by iem_scaled_phase_prepare (idempotent; the number of this program's kernels).
 * The other prepare calls do not prepare it and keep their counts; iem_kernel_info lists these kernels LAST, behind the KKT
 * operator's, with their algorithmic bytes (a phase kernel: the union of its members' reads).  A sharded handle refuses all
 * five calls with IEM_E_ARG (the gradient would need the halo fold and the all-reduce). */
int iem_scaled_phase_prepare(iem_model *m, int32_t *out_n_kernels);
int iem_grad_scaled(iem_model *m, const double *d_x, double obj_scale, double *d_g /* nvar */);
int iem_hess_coord_scaled(iem_model *m, const double *d_x, const double *d_y, const double *d_s /* ncon */,
                          double obj_weight, double *d_vals /* nnzh */);
int iem_eval_trial_scaled(iem_model *m, const double *d_x, const double *d_s /* ncon */, double obj_scale,
                          double *d_c /* ncon */, double *h_obj /* may be NULL */);
int iem_eval_accepted_scaled(iem_model *m, const double *d_x, const double *d_y, const double *d_s /* ncon */,
                             double obj_scale, double obj_weight,
                             double *d_g /* nvar */, double *d_jac /* nnzj */, double *d_hess /* nnzh */);

/* matrix-free products (NLPModels jprod! / jtprod! / hprod!; ExaModels' `prod = true` path —
 * not used by the reference's solvers): Jv (ncon), J'v (nvar), Hv (nvar) with
 * H the Hessian of obj_weight*f + y'c. */
int iem_jprod(iem_model *m, const double *d_x, const double *d_v, double *d_Jv);
int iem_jtprod(iem_model *m, const double *d_x, const double *d_v, double *d_Jtv);
int iem_hprod(iem_model *m, const double *d_x, const double *d_y, const double *d_v, double obj_weight, double *d_Hv);

/* parameter sensitivities: the same three products with d/dθ in place of d/dx, at (x, the handle's current θ — after any
 * iem_set_parameter), L = obj_weight*f + y'c:
 *   iem_jpprod    (dc/dθ) w                        w: npar, out: ncon
 *   iem_jptprod   obj_weight df/dθ + (dc/dθ)' y    y: ncon, out: npar
 *   iem_hpprod    (d2L/dx dθ) w                    w: npar, out: nvar
 * The right-hand side of the first-order parameter step  K [dx; dy] = -[hpprod(δθ); jpprod(δθ)].  One fused kernel per
 * call (plus the deterministic follow-ups of the scatter kinds: no float atomics, bitwise reproducible), the caller's
 * device pointers, outputs fully overwritten, asynchronous on the handle's stream.  Their kernels are a program of their
 * own, generated and loaded by the first such call (iem_kernel_info lists them behind the model's own kernels from then
 * on, kinds 5 / 6 / 7 with names iem_jpprod* / iem_jptprod* / iem_hpprod*).  npar == 0: jpprod and hpprod write zeros,
 * jptprod (a zero-length output) launches nothing.  A sharded handle refuses all three with IEM_E_ARG: θ is replicated on
 * every rank, the products would need an all-reduce.
 * THE FIRST CALL of any of them on a handle sets the program up: it generates the kernels, loads their code object (the
 * cache, else a hiprtc build that can take seconds), allocates and uploads their tables.  That call is therefore
 * synchronous and must not run inside a stream capture; every later call is asynchronous and capturable like the x-kinds.
 * iem_param_prepare does that set-up explicitly (warm up with it before a capture or a timed loop; idempotent) and returns
 * the number of the program's kernels: iem_kernel_info answers for the indices meta.n_kernels .. meta.n_kernels + that
 * number - 1 from then on.  A model the generator refuses stays refused; a runtime failure of the set-up (out of memory, a
 * failed build) is not remembered, the next call tries again. */
int iem_param_prepare(iem_model *m, int32_t *out_n_kernels);
int iem_jpprod(iem_model *m, const double *d_x, const double *d_w, double *d_out);
int iem_jptprod(iem_model *m, const double *d_x, const double *d_y, double obj_weight, double *d_out);
int iem_hpprod(iem_model *m, const double *d_x, const double *d_y, double obj_weight, const double *d_w, double *d_out);
/* the adjoint of iem_hpprod, at the same (x, current θ) and with the same L:
 *   iem_hptprod   (d2L/dθ dx) u                    u: nvar, out: npar
 * With iem_jptprod(obj_weight = 0) it is the product the ADJOINT sensitivity needs: for a quantity q(x, y, θ) of a solution,
 * one solve  K [lx; ly] = [dq/dx; dq/dy]  with the factorised (symmetric) KKT matrix, then
 *   dq/dθ (total) = dq/dθ (partial) - [ hptprod(x, y, lx) + jptprod(x, ly, 0) ]
 * — every entry of θ at the price of one solve, where iem_hpprod / iem_jpprod cost a solve per direction.  One fused kernel
 * (plus the deterministic follow-ups of jptprod's scatter: no float atomics, bitwise reproducible), the output fully
 * overwritten — entries of θ no mixed term reaches get 0 —, asynchronous on the handle's stream.  Its kernels (kind 7, names
 * iem_hptprod*) are one more program of their own, set up by the first iem_hptprod — synchronous, outside a stream capture,
 * like the first call of the three above — or by iem_param_prepare, which prepares BOTH programs and returns the number of
 * kernels of both; iem_kernel_info lists the adjoint kernels behind those of the three kinds above (behind the model's own
 * while only this program exists).  A model without any mixed term has no such kernel: the call is a memset.  npar == 0:
 * nothing is launched.  A sharded handle refuses the call like the three above. */
int iem_hptprod(iem_model *m, const double *d_x, const double *d_y, double obj_weight, const double *d_u, double *d_out);
/* the θθ block of the same L, at the same (x, current θ):
 *   iem_hppprod   (d2L/dθ2) w                      w: npar, out: npar          (d2L/dθ2)' = d2L/dθ2
 * The term the Hessian of the VALUE FUNCTION  φ(θ) = L(x*(θ), y*(θ), θ)  needs beside the products above: with one solve
 *   K [dx; dy] = -[ hpprod(δθ); jpprod(δθ) ]   (the parameter step),
 *   φ''(θ) δθ = hppprod(x, y, δθ) + hptprod(x, y, dx) + jptprod(x, dy, obj_weight = 0)
 * (φ'(θ) = jptprod(x*, y*, obj_weight) by the envelope theorem).  One fused kernel (plus the deterministic follow-ups of
 * jptprod's scatter: no float atomics, bitwise reproducible), the output fully overwritten — entries of θ no θθ term reaches
 * get 0 —, asynchronous on the handle's stream.  Its kernels (kind 7, names iem_hppprod*) are a FOURTH program of their own,
 * set up by the first iem_hppprod — synchronous, outside a stream capture; every later call is asynchronous and capturable —
 * or by iem_hppprod_prepare (idempotent; returns the number of this program's kernels; a runtime failure is not remembered).
 * iem_param_prepare does NOT prepare it and its count does not include it.  iem_kernel_info index rule: the model's own
 * kernels first, then those of every program that exists on the handle in the order  three kinds / adjoint / θθ  — the θθ
 * kernels are always the LAST ones, at  total - n .. total - 1  with n the count iem_hppprod_prepare returns.  A model
 * without a θθ slot (θ read by linear templates only) has no such kernel: the call is a memset.  npar == 0: nothing is
 * launched.  A sharded handle refuses both calls like the four above. */
int iem_hppprod_prepare(iem_model *m, int32_t *out_n_kernels);
int iem_hppprod(iem_model *m, const double *d_x, const double *d_y, double obj_weight, const double *d_w, double *d_out);
/* the three blocks themselves, in COO, at the same (x, current θ) and with the same L:
 *   Jθ  = dc/dθ        ncon x npar   iem_jacp_structure    iem_jacp_coord
 *   Hxθ = d2L/dx dθ    nvar x npar   iem_hessxp_structure  iem_hessp_coord, d_hessxp
 *   Hθθ = d2L/dθ2      npar x npar   iem_hesspp_structure  iem_hessp_coord, d_hesspp
 * What a host with its own linear algebra assembles G = [Hxθ; Jθ] from (K dX = -G, the sensitivity matrix d(x, y)/dθ), and
 * the sparse form of iem_hpprod's output: only the entries that exist are written.
 * PATTERN: symbolic — every kept slot of the model's templates, whatever x, y and θ are; an entry may be numerically zero.
 * iem_param_coord_nnz returns the three lengths {Jθ, Hxθ, Hθθ}; a model without θ, or whose θ no template of a block
 * reads, has 0 there and the call launches nothing for it.
 * SLOT ORDER (the structure calls are the authority): per block, the templates in the order they were added; within a
 * template, item ordinal times the block's slots per item; within an item, the order in which the template's first-order
 * (Jθ) or second-order (Hxθ, Hθθ) slots over the extended vector [x; θ] list the kept ones — a left-to-right, depth-first
 * walk of the expression, first occurrence of an entry (of an ordered pair of entries) opens its slot.  Jθ keeps the θ slots
 * of the constraint templates; Hxθ the second-order slots with exactly one entry in θ; Hθθ those with both; a slot whose
 * entries both lie in x is not part of any block (it belongs to hess_coord!).
 * Hxθ is rectangular: row = the entry of x, column = the entry of θ, whichever operand order the slot has.  Hθθ follows
 * hess_coord!: ONE triangle (row >= col, as iem_hess_structure reports), a slot (a, b) with a != b carries the sum of both
 * orders, a slot whose two θ entries can coincide is doubled where they do, exactly as the Hessian of x handles it; the
 * consumer sums duplicate positions (all three blocks may repeat a position) and mirrors the strict triangle.
 * iem_jacp_coord writes Jθ's values; iem_hessp_coord writes Hxθ's and Hθθ's from ONE second-order sweep (one launch, two
 * output streams).  Either output of iem_hessp_coord may be NULL — required for nothing when its block is empty; for a
 * block with entries the values then go to a spare buffer the handle allocates on the FIRST call that passes NULL for that
 * block, which is therefore synchronous and must stay outside a stream capture like the set-up call — but not both
 * (IEM_E_ARG).  One lane per item, every slot stored exactly once through the store path of jac_coord! / hess_coord!, no
 * atomics, bitwise reproducible from call to call, asynchronous on the handle's stream.  Their kernels (kinds 1 and 2,
 * names iem_jacp* / iem_hessp*) are a FIFTH program of their own, set up by the first iem_jacp_coord / iem_hessp_coord —
 * synchronous, outside a stream capture; every later call is asynchronous and capturable — or by iem_param_coord_prepare
 * (idempotent; returns the number of this program's kernels; a runtime failure of the set-up is not remembered).
 * iem_param_prepare and iem_hppprod_prepare do not prepare it and keep their counts; iem_kernel_info lists these kernels
 * behind those of the other θ programs, in the full order  model / three kinds / adjoint / θθ / θ-COO / residual / scaled
 * (every program that exists on the handle), with their algorithmic bytes read and written.  The
 * structure calls and iem_param_coord_nnz need no program and no device work: they evaluate the index expressions on the
 * host, like iem_jac_structure.  A sharded handle refuses all of them with IEM_E_ARG like the products above. */
int iem_param_coord_prepare(iem_model *m, int32_t *out_n_kernels);
/* how many kernels iem_kernel_info answers for right now: the model's own and those of every further program set up so far */
int iem_kernel_count(const iem_model *m, int32_t *out_total);
int iem_param_coord_nnz(iem_model *m, int64_t out[3]);
int iem_jacp_structure(iem_model *m, int64_t *h_rows, int64_t *h_cols, int base);
int iem_hessxp_structure(iem_model *m, int64_t *h_rows, int64_t *h_cols, int base);
int iem_hesspp_structure(iem_model *m, int64_t *h_rows, int64_t *h_cols, int base);
int iem_jacp_coord(iem_model *m, const double *d_x, double *d_vals);
int iem_hessp_coord(iem_model *m, const double *d_x, const double *d_y, double obj_weight, double *d_hessxp, double *d_hesspp);

/* jac_structure! / hess_structure! — one-off; `base` = 1 for Julia, 0 for C/Python.
 * Hessian pairs are lower-triangular (row >= col); COO may repeat positions. */
int iem_jac_structure(iem_model *m, int64_t *h_rows, int64_t *h_cols, int base);
int iem_hess_structure(iem_model *m, int64_t *h_rows, int64_t *h_cols, int base);
int iem_jac_structure_device(iem_model *m, int64_t *d_rows, int64_t *d_cols, int base);
int iem_hess_structure_device(iem_model *m, int64_t *d_rows, int64_t *d_cols, int base);

/* COO -> CSR value assembly with duplicate summation (the step that follows
 * jac_coord!/hess_coord! in every solver iteration).  `d_perm` lists the COO positions sorted
 * by (row, col); `d_seg[i] .. d_seg[i+1]` delimits the duplicates of CSR nonzero i (n_csr + 1
 * entries).  The plan is built once from the structure (csr.py); this call is per iteration,
 * deterministic (fixed summation order, no atomics). */
int iem_csr_values(iem_model *m, int64_t n_csr, const int64_t *d_seg, const int64_t *d_perm, const double *d_coo,
                   double *d_csr);
/* the same with 32-bit plan words (all COO positions < 2^32): half the plan traffic */
int iem_csr_values32(iem_model *m, int64_t n_csr, const uint32_t *d_seg, const uint32_t *d_perm, const double *d_coo,
                     double *d_csr);

/* y = A x for a CSR matrix with 32-bit indices (the KKT matrix csr.py / kkt.py assemble: residuals for iterative refinement).
 * One thread per row; `d_long_rows` (n_long of them, may be NULL / 0) lists the rows with more than IEM_SPMV_LONG_ROW entries
 * (a first-stage variable's column of J' has one per scenario): those get a workgroup each, summed in a fixed order. */
#define IEM_SPMV_LONG_ROW 256
int iem_csr_spmv(iem_model *m, int64_t n, const int32_t *d_rowptr, const int32_t *d_colind, const double *d_vals, const double *d_x, double *d_y,
                 int64_t n_long, const int64_t *d_long_rows);

/* ---- chain KKT solver (the linear solve that follows jac_coord!/hess_coord! in every interior-point
 * iteration; the reference hands it to MadNLPGPU + CUDSS, README.md:36-37) --------------------------------------------
 * The augmented system of a transcription whose supports couple through a derivative stencil only (transform.jl:535-557)
 * is block tridiagonal once its unknowns are grouped by support, plus a small dense border for finite / first-stage
 * variables — and its coupling blocks are NARROW: K[block k, block k-1] has entries only on a few rows R of block k (the
 * derivative-approximation rows) and a few columns C of block k-1 (the differentiated states), a property block cyclic
 * reduction preserves.  The caller (kkt_chain.py; a Julia host likewise) owns the block arrays on the device and fills
 * them every iteration: D (S x nb x nb, the diagonal blocks, symmetric), Bt (S x nc x nc, Bt[k] = K[block k, block k-1]
 * restricted to rows d_rows[0..nc) of block k and columns d_cols[0..nc) of block k-1; local indices, -1 = padding),
 * E (S x nb x ne, the coupling to the border), row-major.  iem_kkt_chain_factor runs block cyclic reduction in place
 * (hand-written kernels, csrc/iem_kkt_device.h; the inverses on the FP64 matrix cores): D becomes the inverses of the pivot
 * blocks, Bt the couplings of every level, BR (S x nc x nc: the coupling of block i + s to i at the level that eliminated i),
 * Z (as E) and Gp (S x ne x ne, per-block border Schur terms: G_schur = G - sum_k Gp[k]) are outputs; d_info[0] =
 * negative pivots (the inertia), d_info[1] = pivots below `tiny` (replaced by +-tiny: do not trust the factors).
 * iem_kkt_chain_solve: phase 0 reduces the right-hand side r (S x nb, in place; z: S x nb of scratch that must survive until
 * phase 1) and writes rBp (S x ne: r_border_schur = r_border - sum_k rBp[k]); the caller solves the ne x ne border system;
 * phase 1 substitutes back (r becomes the solution).
 * d_Bt == NULL (and d_BR == d_rows == d_cols == d_z == NULL): the blocks couple to the border only (scenario blocks of a
 * two-stage problem) — one launch instead of the levels (ne = -1: no border and a kernel shape for ONE block per launch — the pivot
 * blocks of a dense block factorisation, S = 1).  nb: multiple of 4 in 4..96, ne: multiple of 4 in 0..128, nc: multiple
 * of 4 in 4..48, nc <= nb — and, with a border, the LDS kkt_eliminate declares within the 163 840 bytes of a CU:
 * 8 (2 16R 5 + 2 4 (16R + 1) + 64) + 8 + 8 nb (nb + 1) + 16 nb (ne + 1) with R = ceil(nb / 16) (ne up to 128 for nb <= 60, 64 at
 * nb = 84, 44 at nb = 96); anything else is IEM_E_ARG, from iem_kkt_source as from every call here.  Asynchronous on the handle's stream. */
int iem_kkt_chain_factor(iem_model *m, int64_t S, int nb, int ne, int nc, double *d_D, double *d_Bt, double *d_BR, const int32_t *d_rows,
                         const int32_t *d_cols, double *d_E, double *d_Z, double *d_Gp, int64_t *d_info, double tiny);
/* ONE step of that reduction (no border), for a caller that interleaves work of its own between the levels — the span-sparse
 * border of a laned 2-D grid, kkt_chain.HubChainKKT.  The chain is cut into LANES of lane_len blocks each (S = lanes x lane_len;
 * 0: one chain), every lane reduced by the same levels (block t of a lane leaves at the level s with t mod 2s == s):
 * what = 0 eliminate the blocks t = (2k+1)s of every lane, 1 fold them into the survivors t = 2ks, 2 the last remaining block
 * of every lane (t = 0), 3 clear the pivot counters (d_info).  Levels: s = 1, 2, 4, ... < lane_len. */
int iem_kkt_chain_level(iem_model *m, int64_t S, int64_t lane_len, int nb, int nc, double *d_D, double *d_Bt, double *d_BR, const int32_t *d_rows,
                        const int32_t *d_cols, int64_t *d_info, double tiny, int64_t s, int what);
int iem_kkt_chain_solve(iem_model *m, int64_t S, int nb, int ne, int nc, const double *d_Dinv, const double *d_Bt, const double *d_BR,
                        const int32_t *d_rows, const int32_t *d_cols, const double *d_Z, double *d_r, double *d_z, double *d_rBp,
                        const double *d_xB, int phase);
/* Between two levels of that reduction: the SPAN-SPARSE border columns of the blocks still alive (kkt_chain.HubChainKKT).  A block
 * alive at level s (time block t = a s, a its index among the alive) carries columns for the hubs t - (s - 1) .. t + (s - 1):
 * d_E is [alive][lanes][nq][W], W = (2 s - 1) hw, on the nq local rows d_q that ever hold a border entry (d_qr / d_qc: the
 * positions of the coupling rows / columns inside d_q).  After iem_kkt_chain_level(what = 0) and BEFORE (what = 1):
 * d_Z [eliminated][lanes][nq][W] = D_i^-1[Q, Q] E_i of the blocks just eliminated, d_En [survivors][lanes][nq][(4 s - 1) hw] = the
 * survivors' columns widened by their neighbours' terms.  last != 0: only d_Z for block 0 of every lane (d_E [1][lanes][nq][W]). */
int iem_kkt_hub_level(iem_model *m, int64_t S, int64_t lane_len, int nb, int nc, const double *d_Dinv, const double *d_Bt, const int32_t *d_q, int nq,
                      const int32_t *d_qr, int nr, const int32_t *d_qc, int ncq, int hw, int64_t s, const double *d_E, double *d_Z, double *d_En,
                      int last);
/* ... for factors made lane by lane (iem_kkt_chain_level with lane_len; ne must be 0 when lane_len != S) */
int iem_kkt_chain_solve_lanes(iem_model *m, int64_t S, int64_t lane_len, int nb, int ne, int nc, const double *d_Dinv, const double *d_Bt,
                              const double *d_BR, const int32_t *d_rows, const int32_t *d_cols, const double *d_Z, double *d_r, double *d_z,
                              double *d_rBp, const double *d_xB, int phase);
/* ... and for nrhs right-hand sides at once (csrc/iem_kkt_many_device.h): column u of d_r / d_z is the plane + u S nb, of d_rBp
 * + u S ne, of d_xB + u ne (lane_len = S or 0: one chain).  The columns go through the levels in chunks of 4 (2 for lane-per-row
 * shapes with nc > 16) that read every block of the factors ONCE per level; per column the arithmetic is that of
 * iem_kkt_chain_solve_lanes, operation for operation: the same bits, however the columns are grouped. */
int iem_kkt_chain_solve_many(iem_model *m, int64_t S, int64_t lane_len, int nb, int ne, int nc, const double *d_Dinv, const double *d_Bt,
                             const double *d_BR, const int32_t *d_rows, const int32_t *d_cols, const double *d_Z, double *d_r, double *d_z,
                             double *d_rBp, const double *d_xB, int nrhs, int phase);
/* The dense border on the device (csrc/iem_kkt_border_device.h; the low-level pair behind iem_kkt_set_border(k, 1)).
 * iem_kkt_border_factor: Gs = G - sum_k Gp[k] (G: ne x ne, Gp: S x ne x ne as iem_kkt_chain_factor leaves it; summed by the
 * deterministic two-launch column sum) and, in ONE workgroup with Gs in LDS (8 (ne (ne + 1) + 2 ne + 16) + 4 (2 ne + 16) bytes:
 * 135 360 at ne = 128), an unblocked Bunch-Kaufman LDL' with partial pivoting (alpha = (1 + sqrt 17) / 8, ties to the lowest
 * index): P Gs P' = L D L'.  d_F (ne x ne, row-major): unit L strictly below the diagonal, D on it, the off-diagonal of a 2 x 2
 * pivot in the subdiagonal place, zeros above.  d_piv (ne int32) holds the PERMUTATION and the block structure, not LAPACK's
 * interchange sequence: with p the row of Gs that sits in row i of the factor, d_piv[i] = p for a 1 x 1 pivot, -(p + 1) for the
 * first and -(p + 1) - ne for the second row of a 2 x 2 pivot.  d_info[0] += negative pivots, d_info[1] += doubtful ones (the
 * counters iem_kkt_chain_factor fills; the caller zeroes them otherwise): with scale = max |Gs_ij|, a step whose diagonal entry
 * and column maximum are both <= rel scale (or scale == 0) is doubtful — counted, its pivot replaced by copysign(rel scale, d),
 * its column zeroed and not eliminated (do not trust the factors); a 1 x 1 pivot counts by its sign, a 2 x 2 pivot one negative
 * when its determinant is negative and by the sign of its diagonal otherwise.  n_border: the unknowns in front of the padding's
 * unit diagonal (positive, never counted).
 * iem_kkt_border_solve: xB_u = Gs^-1 (rB_u - sum_k rBp_u[k]) for nrhs columns, one workgroup per column: d_rBp nrhs x S x ne (what
 * phase 0 of iem_kkt_chain_solve / _solve_many writes), d_rB nrhs x ne (entries from n_border on are taken as zero), d_xB nrhs x ne
 * (what phase 1 reads).  Fixed summation order, no atomics: bitwise reproducible.
 * ne: a multiple of 4 in 4..128, 0 <= n_border <= ne, S >= 1, nrhs >= 1 — anything else is IEM_E_ARG before any device work.
 * Both are asynchronous on the handle's stream and capturable once the code object is loaded and the workspace of the column
 * sums (owned by the handle, grown on demand) is large enough: after a first call with the same sizes. */
int iem_kkt_border_factor(iem_model *m, int64_t S, int ne, int n_border, const double *d_G, const double *d_Gp, double *d_F, int32_t *d_piv,
                          int64_t *d_info, double rel);
int iem_kkt_border_solve(iem_model *m, int64_t S, int ne, int n_border, int nrhs, const double *d_F, const int32_t *d_piv, const double *d_rBp,
                         const double *d_rB, double *d_xB);
/* HIP source of those kernels and its cache key — for offline builds (no device needed; malloc'ed) */
int iem_kkt_border_source(char **out_src, uint64_t *out_key);
/* The same solver as ONE object — what a host without the Python layer (a Julia MadNLP linear-solver wrapper) binds.
 * iem_kkt_create analyses the model once on the host: grouping of the unknowns (variable u, then the multiplier of row
 * u - nvar) into chain blocks + border from the slab table and the Jacobian / Hessian structure, the narrow coupling, and a
 * gather plan from the positions of hess_coord! / jac_coord! values to the block entries (duplicates of the COO layout are
 * summed in a fixed order); it owns the device buffers.  Per iteration:
 *   iem_kkt_assemble(k, d_hess, d_jac, d_sigma, delta_w, delta_c)   K = [H + diag(sigma) + delta_w I, J'; J, -delta_c I]
 *                                                                  (d_hess / d_jac: what the handle's iem_hess_coord / iem_jac_coord
 *                                                                   wrote; d_sigma: nvar doubles or NULL)
 *   iem_kkt_factor(k, inertia)        block cyclic reduction + the border's Schur complement; inertia[3] = {positive, negative,
 *                                     doubtful} pivots of K (a correctly regularised system has ncon negative ones); synchronises
 *   iem_kkt_solve(k, d_rhs, d_sol)    K sol = rhs (nvar + ncon doubles each; one pass through the factors — the residual
 *                                     rhs − K sol and iterative refinement: iem_kkt_residual / iem_kkt_solve_refined below)
 * d_rhs and d_sol may be the same array; a PARTIAL overlap of the two is IEM_E_ARG (iem_kkt_solve is iem_kkt_solve_many with one
 * column and takes its rule — such a call used to be undefined, it is refused now).  The object borrows the model handle (its stream, device and kernel cache): destroy
 * it before iem_destroy(m).  Models whose blocks / border / coupling exceed the solver's limits (96 / 64 / 48) are refused by
 * iem_kkt_create. */
typedef struct iem_kkt iem_kkt;
typedef struct {
  int64_t S, n, n_border, block_doubles;   /* blocks, unknowns, border unknowns, doubles of the block buffer D | Bt | E | G */
  int32_t nb, ne, nc, reach, group, phase;
  /* 2-D support grids: lanes > 1 = one chain per point of the other parameter; hubs != 0 = the border (n_border unknowns, ne = 0
   * for the kernels) is kept as span-sparse hub columns: hubs_per_block of them per time block, hub_rows local rows of a block
   * ever hold a border entry, the hubs' Schur complement is a dense matrix with rows of hub_ld doubles */
  int64_t lanes, hub_ld;
  int32_t hubs, hub_rows, hubs_per_block, reserved_;
} iem_kkt_info_t;
int iem_kkt_create(iem_model *m, int group /* 0: the parameter group the stencil runs along */, iem_kkt **out);
int iem_kkt_destroy(iem_kkt *k);
int iem_kkt_info(const iem_kkt *k, iem_kkt_info_t *out);
/* the grouping itself (host arrays; any of them may be NULL): block (-1: border) and place of every unknown, the coupling's rows / columns (nc each, -1 padded) */
int iem_kkt_layout(const iem_kkt *k, int64_t *h_blk, int64_t *h_loc, int32_t *h_rows, int32_t *h_cols);
/* the host analysis alone, from a blob (no device needed; every array malloc'ed — iem_free): the grouping as above and the
 * gather plan  flat[dest[i]] = sum over k in [seg[i], seg[i + 1]) of source(perm[k]),  sources indexing the virtual array
 * hess values | jac values | sigma + delta_w per variable | -delta_c per row | 1.0 (the padding's unit diagonal) */
int iem_kkt_analyse_blob(const void *blob, size_t nbytes, int group, iem_kkt_info_t *info, int64_t **out_blk, int64_t **out_loc, int32_t **out_rows,
                         int32_t **out_cols, int64_t **out_dest, uint32_t **out_seg, uint32_t **out_perm, int64_t *out_n_dest, int64_t *out_n_perm);
int iem_kkt_assemble(iem_kkt *k, const double *d_hess, const double *d_jac, const double *d_sigma, double delta_w, double delta_c);
int iem_kkt_factor(iem_kkt *k, int64_t *out_inertia);
/* Where the dense border (info.ne > 0, no hubs) is factorised and solved.  mode 0 (the default): on the host — iem_kkt_factor
 * brings Gs home for its inertia, every solve synchronises twice and eliminates Gs again.  mode 1: on the device
 * (iem_kkt_border_factor / _solve above): iem_kkt_factor synchronises only to read the counters, and iem_kkt_solve,
 * iem_kkt_solve_many (one border launch per chunk, a workgroup per column; column u still carries the bits of iem_kkt_solve in
 * the same mode) and iem_kkt_solve_refined contain no synchronisation and no copy to or from the host: graph-capturable after
 * their first call.  The inertia is that of a Bunch-Kaufman LDL' in mode 1 (2 x 2 pivots: an indefinite border with a zero
 * diagonal is counted, not reported doubtful).  Switching modes invalidates the factorisation.  A no-op without a dense border
 * (ne == 0, hub mode). */
int iem_kkt_set_border(iem_kkt *k, int mode);
/* iem_kkt_factor without the read-back: {positive, negative, doubtful} into d_inertia (3 int64 on the device) by a one-thread
 * finishing kernel.  No synchronisation; capturable after iem_kkt_set_border(k, 1) (or, without a border, after a first call).
 * IEM_E_ARG in hub mode (its factorisation works on the host between launches) and for ne > 0 in mode 0. */
int iem_kkt_factor_async(iem_kkt *k, int64_t *d_inertia);
int iem_kkt_solve(iem_kkt *k, const double *d_rhs, double *d_sol);
/* K sol_u = rhs_u for nrhs columns with ONE pass over the factors per chunk of columns (sensitivity matrices, several refinement
 * residuals, predictor + corrector): column u is d_rhs + u ld_rhs / d_sol + u ld_sol, nvar + ncon doubles; ld >= nvar + ncon, the
 * entries between are neither read nor written.  d_sol == d_rhs with ld_sol == ld_rhs solves in place; any other overlap is
 * IEM_E_ARG — judged on the whole extents [d, d + (nrhs - 1) ld + n), so columns of d_sol interleaved with those of d_rhs
 * (disjoint, but inside each other's extent) are refused as well.  Any nrhs: the columns are processed in chunks (see iem_kkt_chain_solve_many) through the object's workspace of ONE chunk —
 * one column wide from iem_kkt_create on (a one-column solve allocates nothing), grown once to the chunk width by the first call with
 * nrhs > 1, freed by iem_kkt_destroy: memory does not grow with nrhs.  THE GROWTH FREES the one-column buffers: a graph captured
 * from iem_kkt_solve / iem_kkt_solve_refined before it points at freed memory afterwards — an application that uses both kinds of
 * call makes one multi-column call before it captures, or captures again after the first one.  iem_kkt_solve is this call with one column: column u carries
 * the bits iem_kkt_solve gives for it.  In mode 0 the border system is solved on the host once per column, with one read-back and one upload per
 * chunk; in mode 1 (iem_kkt_set_border) on the device, one launch per chunk.  Hub mode (info.hubs != 0) is accepted as a loop of single solves: the hubs' side stays matrix-vector work per column
 * (sharing its factors across columns — GEMM for GEMV — is not done). */
int iem_kkt_solve_many(iem_kkt *k, int nrhs, const double *d_rhs, int64_t ld_rhs, double *d_sol, int64_t ld_sol);

/* HIP source of the solver's kernels for one (nb, ne, nc) and its cache key — for offline builds (no device needed; malloc'ed).
 * A shape iem_kkt_chain_factor refuses is refused here with the same IEM_E_ARG and the same message. */
int iem_kkt_source(int nb, int ne, int nc, char **out_src, uint64_t *out_key);

/* r = rhs − K sol  with  K = [W + diag(sigma) + delta_w I, J'; J, −delta_c I]  at (x, y, obj_weight) — matrix-free: iem_kktprod
 * on the borrowed model handle (K0 sol into a workspace of nvar + ncon doubles that the first call allocates and iem_kkt_destroy
 * frees) and ONE finishing kernel that computes, without contraction and in this order,
 *     r_x = rhs_x − (p_x + (sigma + delta_w) ∘ sol_x),     r_y = rhs_y − (p_y − delta_c · sol_y)
 * and — d_norm != NULL — the device scalar max_i |r_i|: an integer maximum over the bit patterns (a NaN in r gives a NaN), order-
 * independent and bitwise reproducible.  d_sigma: nvar doubles or NULL.  d_r may be d_rhs; no other overlap.  The factors are not
 * touched: every mode of the object (1-D chain, lanes, hubs), factorised or not.  Asynchronous and capturable after the first
 * call (or after iem_kktprod_prepare and one call). */
int iem_kkt_residual(iem_kkt *k, const double *d_x, const double *d_y, double obj_weight, const double *d_sigma /* nvar or NULL */,
                     double delta_w, double delta_c, const double *d_rhs, const double *d_sol, double *d_r, double *d_norm);
/* sol = solve(rhs); then `steps` times  r = residual(sol), sol += solve(r)  — each step bitwise what iem_kkt_solve,
 * iem_kkt_residual and a vector add give.  d_norms (steps + 1 doubles or NULL): d_norms[i] = max |r| in front of step i, the
 * last entry the one behind the last step (with d_norms == NULL that last residual is not computed).  steps = 0 is iem_kkt_solve
 * (plus one norm).  No host read-back of a norm and no early exit: as asynchronous and capturable as iem_kkt_solve itself is for
 * the object (a dense border is solved on the host in mode 0 only: iem_kkt_set_border).  d_sol may not overlap d_rhs.  Workspace: 3 (nvar + ncon) doubles, as above. */
int iem_kkt_solve_refined(iem_kkt *k, const double *d_x, const double *d_y, double obj_weight, const double *d_sigma, double delta_w,
                          double delta_c, const double *d_rhs, double *d_sol, int steps, double *d_norms /* steps + 1 or NULL */);

/* A PER-ROW diagonal in the constraint block — what an interior-point method with eliminated slacks assembles (Sigma_s^-1 on its
 * inequality rows, another value per row at every iterate) — and the residual / refinement over several columns:
 *     K = [W + diag(sigma) + delta_w I, J'; J, −diag(dcon + delta_c)]          (delta_c is added on EVERY row, as Ipopt's is)
 * d_dcon: ncon doubles on the device, or NULL = zeros; ignored when ncon == 0.  Its entries are NOT inspected — none of the
 * calls synchronises —: a negative or NaN entry goes into the matrix (and into the residuals) as it is.
 * iem_kkt_assemble_diag: iem_kkt_assemble with the per-row source −(dcon[row] + delta_c) (one rounded add, then the negation;
 * every other source and the summation order are unchanged), in every mode of the object (1-D chain, lanes with a dense border
 * in both border modes, hubs); d_dcon == NULL is iem_kkt_assemble itself.  Invalidates the factorisation.
 * iem_kkt_residual_diag: r_u = rhs_u − K sol_u for nrhs columns (column u at d + u ld; ld >= nvar + ncon, the entries between the
 * columns are neither read nor written): one iem_kktprod per column into a workspace plane, then ONE finishing launch per slab
 * of 8 columns that computes, without contraction and in this order,
 *     r_x = rhs_x − (p_x + (sigma + delta_w) ∘ sol_x),     d = dcon + delta_c (delta_c alone for d_dcon == NULL),  r_y = rhs_y − (p_y − d ∘ sol_y)
 * and — d_norms != NULL — d_norms[u] = max_i |r_u[i]| as iem_kkt_residual forms it (integer maximum on the bit patterns: a NaN
 * gives a NaN, order-independent).  With nrhs = 1 and d_dcon == NULL: the bits of iem_kkt_residual.  Column u carries the bits of
 * the call on that column alone.  d_r may be d_rhs when ld_r == ld_rhs; every other overlap of d_r, d_sol, d_rhs, d_norms —
 * judged on the whole extents [d, d + (nrhs − 1) ld + n), as for iem_kkt_solve_many — is IEM_E_ARG.  A sharded model handle is
 * refused where iem_kktprod refuses it.
 * iem_kkt_solve_refined_diag: iem_kkt_solve_many, then `steps` times: the residuals, iem_kkt_solve_many on them, ONE add kernel
 * (sol_u += dsol_u).  d_norms ((steps + 1) nrhs doubles or NULL): d_norms[i nrhs + u] = max |r_u| in front of step i, the last row
 * the one behind the last step (with d_norms == NULL that last residual is not formed).  steps >= 0.  No read-back of a norm and
 * no early exit: as asynchronous and capturable as iem_kkt_solve_many is for the object's mode, after a first call.  d_sol may
 * not overlap d_rhs (nor d_norms either).  With nrhs = 1 and d_dcon == NULL: the bits of iem_kkt_solve_refined.
 * iem_kkt_assemble, iem_kkt_residual and iem_kkt_solve_refined ARE these calls with nrhs = 1, ld = nvar + ncon and d_dcon == NULL.
 * Workspace: 3 (nvar + ncon) doubles per column, owned by the object and shared by the residual and refined calls: one column from
 * the first such call on, ONE slab (8 columns — a multiple of every chunk width of iem_kkt_solve_many) from the first call with
 * nrhs > 1 on (the growth waits for the stream once and frees the one-column planes: a graph captured from iem_kkt_residual /
 * iem_kkt_solve_refined before it has to be captured again, as for iem_kkt_solve_many); freed by iem_kkt_destroy; it does not grow
 * with nrhs. */
int iem_kkt_assemble_diag(iem_kkt *k, const double *d_hess, const double *d_jac, const double *d_sigma /* nvar | NULL */,
                          const double *d_dcon /* ncon | NULL */, double delta_w, double delta_c);
int iem_kkt_residual_diag(iem_kkt *k, const double *d_x, const double *d_y, double obj_weight, const double *d_sigma,
                          const double *d_dcon, double delta_w, double delta_c, int nrhs,
                          const double *d_rhs, int64_t ld_rhs, const double *d_sol, int64_t ld_sol,
                          double *d_r, int64_t ld_r, double *d_norms /* nrhs | NULL */);
int iem_kkt_solve_refined_diag(iem_kkt *k, const double *d_x, const double *d_y, double obj_weight, const double *d_sigma,
                               const double *d_dcon, double delta_w, double delta_c, int nrhs,
                               const double *d_rhs, int64_t ld_rhs, double *d_sol, int64_t ld_sol,
                               int steps, double *d_norms /* (steps + 1)·nrhs | NULL; entry [i·nrhs + u] */);
/* HIP source of kkt_gather_d / kkt_residual_dm / kkt_axpy_m and its cache key — for offline builds (no device needed; malloc'ed) */
int iem_kkt_diag_source(char **out_src, uint64_t *out_key);

/* ---- the interior-point barrier layer -------------------------------------------------------------------------------------------
 * What sits between the evaluation calls and the KKT object in a primal-dual interior-point iteration (Ipopt / MadNLP with
 * eliminated slacks), as an object beside iem_kkt: the barrier diagonal, the condensed right-hand side, the slack and bound-
 * multiplier directions, the fraction-to-the-boundary step lengths, the update with the multiplier safeguard, Ipopt's error terms.
 * Sign convention  grad f + J'y − zL + zU = 0.  Rows with lcon == ucon are equalities (c = ceq); every other row is an inequality
 * with an eliminated slack s:  c − s = 0,  rl <= s <= ru.  Relaxed bounds, formed on the host at create time:
 *     xl = lvar − relax·max(1, |lvar|),  xu = uvar + relax·max(1, |uvar|)  where finite (∓inf otherwise);  rl / ru likewise from the
 *     lcon / ucon of inequality rows;  ceq = lcon, unrelaxed.
 * State vectors are FULL LENGTH, nothing is compacted: x, zL, zU (and dzL, dzU) have nvar entries; s, vL, vU, ds, dvL, dvU have ncon
 * entries of which those on equality rows are never read and never written.  zL[i] / zU[i] / vL[j] / vU[j] are read only where that
 * bound is present (a finite relaxed bound — for v*: of an inequality row).  An absent bound contributes an exact +0.0.
 * Gaps  dL = x − xl, dU = xu − x, eL = s − rl, eU = ru − s.  Every operation below is rounded once, in the order written (the code
 * object is compiled with -ffp-contract=off):
 *     sigma_i = (hasL ? zL/dL : 0) + (hasU ? zU/dU : 0)        gb_i = (hasU ? mu/dU : 0) − (hasL ? mu/dL : 0)     rhs_x_i = −(r_i + gb_i)
 *     sigs_j  = (gL ? vL/eL : 0) + (gU ? vU/eU : 0)            gs_j = (gU ? mu/eU : 0) − (gL ? mu/eL : 0)
 *     rs_j    = gs_j − y_j                                     inv_j = 1.0/sigs_j
 *     equality row:    dcon_j = 0.0     rhs_y_j = −(c_j − ceq_j)
 *     inequality row:  dcon_j = inv_j   rhs_y_j = −((c_j − s_j) + rs_j·inv_j)
 *     ds_j  = (dy_j − rs_j)/sigs_j                                                                 (inequality rows)
 *     dzL_i = hasL ? (mu/dL − zL) − (zL/dL)·dx : 0             dzU_i = hasU ? (mu/dU − zU) + (zU/dU)·dx : 0
 *     dvL_j, dvU_j: the same with (eL, eU, vL, vU, ds)
 * K = [W + diag(sigma) + delta_w I, J'; J, −diag(dcon + delta_c)] with this rhs is the system iem_kkt_assemble_diag /
 * iem_kkt_solve_refined_diag solve; sol = [dx; dy].  r = obj_weight·grad f + J'y is what iem_eval_residual writes.
 *
 * iem_barrier_create: h_lvar / h_uvar (nvar) and h_lcon / h_ucon (ncon) host arrays, each NULL = the handle's own mirror
 *     (iem_get_host); a scaled solver passes its scaled row bounds.  Loads the code object (first object of the handle), uploads
 *     the bounds, allocates everything the calls below use.  IEM_E_ARG: a sharded handle, relax < 0, relax == 0 with a fixed
 *     variable (lvar == uvar), a row with neither bound, lvar > uvar or lcon > ucon.  The object borrows the model handle (stream,
 *     device, kernel cache): destroy it before iem_destroy(m).
 * iem_barrier_start:  Ipopt's bound_push / bound_frac projection, for a bound pair (lo, hi) of which `both` are present:
 *     pl = bound_push·max(|lo|, 1), pu = bound_push·max(|hi|, 1), both: pl = min(pl, bound_frac·(hi − lo)), pu likewise;
 *     v = max(v, lo + pl) where lo is present, then v = min(v, hi − pu) where hi is.  x is projected in place, s = that projection of
 *     c on inequality rows; zL, zU = 1.0 where present and 0.0 elsewhere, vL, vU likewise on inequality rows.
 * iem_barrier_terms:  sigma (nvar), dcon (ncon), rhs (nvar + ncon) as above.
 * iem_barrier_step:   ds, dzL, dzU, dvL, dvU from d_sol = [dx; dy], and d_alpha[0] = alpha_primal, d_alpha[1] = alpha_dual:
 *     alpha = min(1, candidates) with the candidates ((−tau)·gapL)/d where d < 0 and the lower bound is present, (tau·gapU)/d where
 *     d > 0 and the upper bound is present (d = dx on x, ds on s), and ((−tau)·z)/dz where dz < 0 for the four multiplier vectors.
 *     The minimum is an integer minimum on the bit patterns (order-independent; the slots are seeded with the bits of 1.0 by a
 *     device-to-device copy).  A candidate that is not > 0 — a NaN or non-positive gap in the state, met by a direction that moves
 *     towards that bound — enters as +0.0, and so does a NaN anywhere in a direction: in dx, dy or ds for alpha_primal, in dzL, dzU,
 *     dvL or dvU (present bounds) for alpha_dual.  (A point exactly on a bound with a direction that leaves it inwards gives no
 *     candidate; its sigma is inf.)  ALPHA = +0.0 MEANS THE STATE OR THE DIRECTION WAS UNUSABLE, and
 * iem_barrier_update with either step length +0.0 writes nothing: every state bit stays.  Otherwise  x += alpha_p·dx,
 *     s += alpha_p·ds, y += alpha_p·dy, z* += alpha_d·dz*, v* += alpha_d·dv*  (the step lengths read from d_alpha on the device) and
 *     then, with the NEW gaps, per present bound  z = min(max(z, mu/(kappa_sigma·gap)), (kappa_sigma·mu)/gap).
 * iem_barrier_error:  d_out[0] = max_i |r − zL + zU|, [1] = max_j |−y − vL + vU| over inequality rows, [2] = max_j |infeasibility|
 *     (c − ceq on equality rows, c − s on inequality rows), [3] = max |gap·z − mu| over present bounds, [4] = sum |y|, [5] = sum of
 *     the present multipliers, [6] = theta = sum_j |infeasibility|, [7] = sum log gap over present bounds.  The maxima are integer
 *     maxima on the bit patterns (a NaN wins); the sums are reduced in a fixed order (per workgroup, then by the workgroup that
 *     finishes last): bitwise reproducible, no float atomic.  d_r == NULL: d_out[0] is written as NaN.
 * iem_barrier_merit:  d_out[0] = theta, d_out[1] = sum log gap at a trial (x, s, c): the bits iem_barrier_error writes to [6], [7].
 * All six run on the handle's stream, one launch each (step: a 16-byte copy in front, error: a 32-byte memset), asynchronous, without
 * synchronisation, allocation or host copy: graph-capturable.  Entries of the device vectors are never inspected.  IEM_E_ARG before
 * any device work: null required pointers (s, vL, vU, ds, dvL, dvU may be NULL without inequality rows; y, c, dcon without rows),
 * tau outside (0, 1], mu < 0, kappa_sigma < 1, bound_push <= 0, bound_frac outside (0, 0.5]. */
typedef struct iem_barrier iem_barrier;
typedef struct {
  uint64_t struct_size;                 /* set by the CALLER to sizeof(iem_barrier_info_t): at most that many bytes are written */
  int64_t nvar, ncon, n_eq, n_ineq;
  int64_t n_xl, n_xu, n_sl, n_su;       /* present lower / upper bounds of x, of the inequality rows' slacks */
  int64_t nz;                           /* their sum: the number of bound multipliers */
  int64_t workgroups;                   /* of every launch (256 threads each, grid-stride over nvar + ncon entries) */
} iem_barrier_info_t;
int iem_barrier_create(iem_model *m, const double *h_lvar, const double *h_uvar, const double *h_lcon, const double *h_ucon, double relax, iem_barrier **out);
/* the host analysis alone (no device needed), with iem_barrier_create's refusals: h_bounds (2 nvar + 3 ncon doubles) = xl | xu | rl | ru |
 * ceq (rl / ru = ∓inf and ceq = lcon on equality rows, ceq = 0 elsewhere), h_flags (nvar + ncon bytes): bit 0 / 1 = the lower / upper
 * bound is present, bit 2 = equality row; info as iem_barrier_info fills it */
int iem_barrier_analyse(int64_t nvar, int64_t ncon, const double *h_lvar, const double *h_uvar, const double *h_lcon, const double *h_ucon, double relax,
                        double *h_bounds, uint8_t *h_flags, iem_barrier_info_t *info);
int iem_barrier_destroy(iem_barrier *b);
int iem_barrier_info(const iem_barrier *b, iem_barrier_info_t *out);
int iem_barrier_start(iem_barrier *b, double *d_x, const double *d_c, double *d_s, double *d_zL, double *d_zU, double *d_vL, double *d_vU, double bound_push,
                      double bound_frac);
int iem_barrier_terms(iem_barrier *b, const double *d_x, const double *d_s, const double *d_y, const double *d_zL, const double *d_zU, const double *d_vL,
                      const double *d_vU, const double *d_r, const double *d_c, double mu, double *d_sigma, double *d_dcon, double *d_rhs);
int iem_barrier_step(iem_barrier *b, const double *d_x, const double *d_s, const double *d_y, const double *d_zL, const double *d_zU, const double *d_vL,
                     const double *d_vU, const double *d_sol, double mu, double tau, double *d_ds, double *d_dzL, double *d_dzU, double *d_dvL, double *d_dvU,
                     double *d_alpha /* 2 */);
int iem_barrier_update(iem_barrier *b, double *d_x, double *d_s, double *d_y, double *d_zL, double *d_zU, double *d_vL, double *d_vU, const double *d_sol,
                       const double *d_ds, const double *d_dzL, const double *d_dzU, const double *d_dvL, const double *d_dvU, const double *d_alpha, double mu,
                       double kappa_sigma);
int iem_barrier_error(iem_barrier *b, const double *d_x, const double *d_s, const double *d_y, const double *d_zL, const double *d_zU, const double *d_vL,
                      const double *d_vU, const double *d_r /* nvar | NULL */, const double *d_c, double mu, double *d_out /* 8 */);
int iem_barrier_merit(iem_barrier *b, const double *d_x, const double *d_s, const double *d_c, double *d_out /* 2 */);
/* HIP source of the six kernels and its cache key — for offline builds (no device needed; malloc'ed) */
int iem_barrier_source(char **out_src, uint64_t *out_key);

/* ---- the filter line search ------------------------------------------------------------------------------------------------------
 * The decision of an interior-point iteration on the device (csrc/iem_search_device.h), as an object beside iem_barrier: the slope of
 * the barrier objective phi_mu = obj_weight·f − mu·sum log gap along the direction, the trial point, and the acceptance test of
 * Waechter and Biegler 2006, Algorithm A, with its filter.  A ladder of K rungs
 *     iem_search_begin;  K × { iem_search_trial, iem_obj_device, iem_cons, iem_barrier_merit, iem_search_accept };  iem_barrier_update
 * needs no host decision and is graph-capturable: once a rung accepts, the later rungs recompute the same trial point and their
 * accept call returns at its first test; iem_barrier_update moves nothing for alpha = +0.0, which is what a search without a step
 * leaves in d_alpha[0].  The host reads one status word (iem_search_state, or its own copy of the block) when it likes.
 *
 * THE CONTROL BLOCK: sixteen 8-byte words on the device (iem_search_device gives the pointer; a host may write word 0 or word 9):
 *     0 alpha (double)          1 alpha_max: the d_alpha[0] that begin saw      2 phi0 = obj_weight·f − mu·sum log gap      3 theta0
 *     4 slope                   5 theta_min      6 theta_max                    7 phi of the last trial   8 theta of the last trial
 *     9 status (int64): 0 SEARCHING, 1 accepted f-type, 2 accepted h-type, 3 FAILED, 4 UNUSABLE           10 trials (int64)
 *     11 filter count (int64)   12 flags (int64): bit 0 = theta_min / theta_max are set, bit 1 = filter overflow        13–15 zero (begin) — the iem_soc object's
 * The filter: filter_capacity pairs (theta, phi) on the device, the first `filter count` of them in use.
 *
 * iem_search_begin: slope = sum of  t_i = (obj_weight·g_i + gb_i)·dx_i  over the variables and  t_j = gs_j·ds_j  over the inequality
 *     rows (gb_i, gs_j of the barrier contract above: the same gaps, the same branches for absent bounds, the same rounding order;
 *     equality rows are skipped, their ds entries never read); d_grad = grad f as iem_grad / iem_eval_accepted write it.  A lane adds its entries
 *     in index order, the workgroups' totals are summed in the fixed order of the barrier sums: bitwise reproducible, no float
 *     atomic.  The workgroup that arrives last fills words 0–4, 7–10 and 13–15: alpha = alpha_max = d_alpha[0], phi0 from d_obj[0] and
 *     d_err[7], theta0 = d_err[6], trials = 0, words 7 and 8 NaN, status SEARCHING — or UNUSABLE with alpha = +0.0 when d_alpha[0] is not
 *     > 0 (+0.0: the barrier layer's "unusable") or the slope is NaN.  While flag bit 0 is clear it sets theta_min = 1e-4·max(1, theta0),
 *     theta_max = 1e4·max(1, theta0) and the bit.  The filter, its count and flag bit 1 stay.
 * iem_search_trial:  xt = x + alpha·dx,  st = s + alpha·ds on inequality rows (equality rows' entries never written), alpha read from
 *     the block; with status FAILED or UNUSABLE nothing is stored.
 * iem_search_accept: ONE workgroup of 64 threads.  With a status other than SEARCHING it writes only d_alpha[0] — the accepted alpha,
 *     or +0.0 for FAILED / UNUSABLE.  Otherwise, each operation rounded once:  theta_t = d_merit[0],  phi_t = obj_weight·ft − mu·d_merit[1];
 *         admissible:  phi_t and theta_t finite, theta_t <= theta_max, and no filter entry (Ft, Fp) with theta_t >= Ft and phi_t >= Fp
 *         switching:   slope < 0 and theta0 <= theta_min and alpha·pow(−slope, s_phi) > delta·pow(theta0, s_theta)
 *         Armijo:      phi_t <= (phi0 + (eta_phi·alpha)·slope) + (10·2⁻⁵²)·|phi0|
 *         sufficient:  theta_t <= (1 − gamma_theta)·theta0  or  phi_t <= phi0 − gamma_phi·theta0
 *     admissible, switching, Armijo: accepted, status 1;  admissible, not switching, sufficient: accepted, status 2 — and then the filter
 *     gains ((1 − gamma_theta)·theta0, phi0 − gamma_phi·theta0): the entries it dominates (both coordinates >=) leave first, the others
 *     keep their order, the new entry is appended; a full filter sets flag bit 1 and appends nothing, the step still stands (entries
 *     behind the count are not defined).  Accepted: d_alpha[0] = alpha.  Rejected: trials += 1, alpha = 0.5·alpha, d_alpha[0] = +0.0; if trials ==
 *     max_trials or the new alpha < alpha_floor the status becomes FAILED and alpha +0.0.  Words 7, 8 take phi_t, theta_t either way.
 *     d_alpha[1] (the dual step length) is never touched.
 * iem_search_reset: a new barrier problem (mu changed): filter emptied, flags cleared — one asynchronous 16-byte memset.
 * Every call runs on the handle's stream; begin, trial and accept are one launch each; nothing allocates after create, nothing
 * synchronises and nothing is copied to the host, except by iem_search_state.  IEM_E_ARG before any device work: null required
 * pointers (s, ds, st may be NULL without inequality rows), mu < 0, options out of range (gamma_theta, gamma_phi, eta_phi in (0, 1),
 * delta > 0, s_theta > 1, s_phi >= 1, alpha_floor >= 0, max_trials >= 1, 1 <= filter_capacity <= 1024).  The object borrows the barrier object (bounds,
 * flags, grid) and through it the model handle: destroy it before them.  Not here: inertia correction (the mu update is the iem_mu object below),
 * sharded handles (iem_barrier_create refuses them); restoration is the iem_resto object below, Ipopt's alpha_min rule iem_rmu_trigger.  The second-order correction is the
 * iem_soc object below; words 13–15 of the block are its. */
typedef struct iem_search iem_search;
typedef struct {
  uint64_t struct_size;                 /* set by the CALLER to sizeof(iem_search_opts_t) */
  double gamma_theta, gamma_phi, eta_phi, delta, s_theta, s_phi, alpha_floor;
  int64_t max_trials, filter_capacity;
} iem_search_opts_t;                    /* NULL = Ipopt's defaults: 1e-5, 1e-8, 1e-8, 1.0, 1.1, 2.3, 1e-16, 30, 64 */
typedef struct {
  uint64_t struct_size;                 /* set by the CALLER to sizeof(iem_search_state_t): at most that many bytes are written */
  double alpha, alpha_max, phi0, theta0, slope, theta_min, theta_max, phi_trial, theta_trial;      /* words 0–8 of the block */
  int64_t status, trials, filter_count, flags;                                                     /* words 9–12 */
} iem_search_state_t;
enum { IEM_SEARCH_SEARCHING = 0, IEM_SEARCH_F_TYPE = 1, IEM_SEARCH_H_TYPE = 2, IEM_SEARCH_FAILED = 3, IEM_SEARCH_UNUSABLE = 4 };
int iem_search_create(iem_barrier *b, const iem_search_opts_t *opts, iem_search **out);
int iem_search_destroy(iem_search *s);
int iem_search_reset(iem_search *s);
int iem_search_begin(iem_search *s, const double *d_x, const double *d_s, const double *d_grad, const double *d_sol, const double *d_ds,
                     const double *d_obj, const double *d_err /* 8, of iem_barrier_error at this point */, const double *d_alpha /* 2 */,
                     double mu, double obj_weight);
int iem_search_trial(iem_search *s, const double *d_x, const double *d_s, const double *d_sol, const double *d_ds, double *d_xt, double *d_st);
int iem_search_accept(iem_search *s, const double *d_ft, const double *d_merit /* 2 */, double mu, double obj_weight, double *d_alpha);
int iem_search_device(const iem_search *s, void **d_control, double **d_filter /* filter_capacity pairs (theta, phi) */);
int iem_search_state(iem_search *s, iem_search_state_t *out);      /* synchronises the stream: the one read-back */
/* HIP source of the three kernels and its cache key — for offline builds (no device needed; malloc'ed) */
int iem_search_source(char **out_src, uint64_t *out_key);

/* ---- the second-order correction of the filter line search -----------------------------------------------------------------------
 * Waechter and Biegler 2006, Algorithm A, steps A-5.5 to A-5.9 (Ipopt's TrySecondOrderCorrection, max_soc = 4, kappa_soc = 0.99) on the
 * device (csrc/iem_soc_device.h), as an object beside iem_search: between the first rejected trial and the first halving of alpha, the
 * constraint residual of the rejected trial point is added to the right-hand side and the corrected step is tested at full length.
 * Every call is ONE launch and is gated ON THE DEVICE by words 13–15 of the search object's control block, so the same sequence serves a
 * host that reads the status word after the first rung and runs the rounds only when wanted, and a captured ladder that holds P rounds
 * unconditionally — a call that does not apply returns before its first store:
 *     iem_search_begin;  rung;  iem_soc_open;
 *     P × { iem_soc_rhs, iem_kkt_solve_refined_diag(1 column: rhs_soc -> sol_soc), iem_barrier_step(sol_soc -> ds_soc, dzL_soc, dzU_soc,
 *           dvL_soc, dvU_soc, alpha_soc), iem_soc_trial, iem_obj_device, iem_cons, iem_barrier_merit, iem_soc_accept };
 *     iem_soc_select;  (K − 1) × rung;  iem_barrier_update
 * (rung = { iem_search_trial, iem_obj_device, iem_cons, iem_barrier_merit, iem_search_accept }).  The solve and the step run on this
 * iteration's factors and are unchanged; while the correction is not ACTIVE they compute on buffers nobody reads.
 *
 * THE CONTROL BLOCK, words 13–15 (iem_search_begin zeroes them for every search):
 *     13 state (int64): 0 NONE, 1 ACTIVE, 2 ACCEPTED, 3 CLOSED      14 rounds finished (int64)      15 alpha_prev (double)
 *
 * iem_soc_open: one workgroup; behind the first rung's iem_search_accept.  With state NONE: ACTIVE when status == SEARCHING, trials == 1
 *     and theta of the last trial (word 8) is finite and >= theta0 (word 3) (a NaN compares false) — then rounds = 0 and alpha_prev =
 *     alpha_max (word 1); otherwise CLOSED.  With any other state it writes nothing (idempotent: a replayed graph finds it decided).
 *     A search with max_trials = 1 has FAILED at its first rejection, before a correction can open.
 * iem_soc_rhs: with state ACTIVE, per row j (inf_t_j = ct_j − ceq_j on an equality row, ct_j − st_j on an inequality row: the
 *     infeasibility of iem_barrier_merit at the latest trial point; each operation rounded once, in the order written):
 *         rounds == 0:  prev_j = c_j − ceq_j  resp.  c_j − s_j          rounds > 0:  prev_j = csoc_j
 *         csoc_j = alpha_prev·prev_j + inf_t_j                          (a product, then a sum; csoc is stored in the object)
 *         equality row:    rhs_soc_y_j = −csoc_j
 *         inequality row:  rhs_soc_y_j = −(csoc_j + rs_j·inv_j)         rs_j, inv_j of the barrier contract above from (s, y, vL, vU, mu)
 *     and rhs_soc_i = rhs_i for i < nvar (the bits copied).  Only the linearised constraint J·dx − ds = −(c − s) changes: ds = (dy − rs)/sigs
 *     and every multiplier direction keep their formulas, so iem_barrier_step is the step of the corrected direction.  Not ACTIVE:
 *     nothing is stored, csoc stays.
 * iem_soc_trial: with state ACTIVE and alpha_soc[0] > 0:  xt = x + alpha_soc[0]·dx_soc,  st = s + alpha_soc[0]·ds_soc on inequality rows
 *     (equality rows' entries never written); otherwise nothing is stored.
 * iem_soc_accept: ONE workgroup of 64 threads.  Not ACTIVE: writes nothing at all.  ACTIVE with alpha_soc[0] not > 0 (the barrier
 *     layer's "unusable"): state CLOSED, rounds += 1, nothing else.  Otherwise the test of iem_search_accept word for word — theta_t,
 *     phi_t, admissible, switching, Armijo, sufficient, in that rounding order — with alpha := alpha_max (word 1) in the switching
 *     condition and in Armijo (Ipopt tests a corrected step with the full step's alpha).  Words 7, 8 take phi_t, theta_t and rounds += 1
 *     either way.  Accepted: status 1 (f-type) or 2 (h-type: the filter gains its entry exactly as in iem_search_accept, overflow flag
 *     included), word 0 = alpha_soc[0], d_alpha[0] = alpha_soc[0], d_alpha[1] = alpha_soc[1], state ACCEPTED.  Rejected: with p = the new
 *     rounds, the correction goes on iff p < max_soc and theta_t is finite and theta_t <= kappa_soc·theta_prev (theta_prev = word 8 before
 *     this call: the previous trial's theta; one product) — then alpha_prev = alpha_soc[0]; otherwise state CLOSED, and backtracking
 *     continues from alpha_max/2, which the rejecting iem_search_accept left in word 0.  A rejection touches neither status, trials,
 *     word 0 nor d_alpha.
 * iem_soc_select: iff state ACCEPTED it copies the corrected direction over the first-order one — sol: nvar + ncon entries, dzL, dzU:
 *     nvar, ds, dvL, dvU: inequality rows only; otherwise nothing.  The later rungs' iem_search_trial then recomputes x + alpha_soc·dx_soc
 *     from the expression of iem_soc_trial (the same bits), and iem_barrier_update takes the corrected step with no host decision.
 * Every call runs on the handle's stream, one launch, asynchronous, capturable; nothing allocates after create, nothing synchronises
 * and nothing is copied to the host, except by iem_soc_state.  IEM_E_ARG before any device work: null required pointers (s, y, vL, vU,
 * st, ds*, dvL*, dvU* may be NULL without inequality rows), mu < 0, max_soc outside [1, 16], kappa_soc outside (0, 1].  The object
 * borrows the search object (block, filter, options) and through it the barrier object: destroy it before them.  Not here: the mu
 * update, inertia correction, sharded handles (restoration: the iem_resto object below). */
typedef struct iem_soc iem_soc;
typedef struct {
  uint64_t struct_size;                 /* set by the CALLER to sizeof(iem_soc_opts_t) */
  int64_t max_soc;
  double kappa_soc;
} iem_soc_opts_t;                       /* NULL = Ipopt's defaults: 4, 0.99 */
typedef struct {
  uint64_t struct_size;                 /* set by the CALLER to sizeof(iem_soc_state_t): at most that many bytes are written */
  int64_t status;                       /* word 9 of the block */
  int64_t state, rounds;                /* words 13, 14 */
  double alpha_prev;                    /* word 15 */
} iem_soc_state_t;
enum { IEM_SOC_NONE = 0, IEM_SOC_ACTIVE = 1, IEM_SOC_ACCEPTED = 2, IEM_SOC_CLOSED = 3 };
int iem_soc_create(iem_search *s, const iem_soc_opts_t *opts, iem_soc **out);      /* allocates csoc (ncon doubles, zeroed) */
int iem_soc_destroy(iem_soc *q);
int iem_soc_open(iem_soc *q);
int iem_soc_rhs(iem_soc *q, const double *d_s, const double *d_y, const double *d_vL, const double *d_vU, const double *d_c, const double *d_ct,
                const double *d_st, const double *d_rhs, double mu, double *d_rhs_soc);
int iem_soc_trial(iem_soc *q, const double *d_x, const double *d_s, const double *d_sol_soc, const double *d_ds_soc, const double *d_alpha_soc /* 2 */,
                  double *d_xt, double *d_st);
int iem_soc_accept(iem_soc *q, const double *d_ft, const double *d_merit /* 2 */, const double *d_alpha_soc /* 2 */, double mu, double obj_weight,
                   double *d_alpha /* 2 */);
int iem_soc_select(iem_soc *q, const double *d_sol_soc, const double *d_ds_soc, const double *d_dzL_soc, const double *d_dzU_soc, const double *d_dvL_soc,
                   const double *d_dvU_soc, double *d_sol, double *d_ds, double *d_dzL, double *d_dzU, double *d_dvL, double *d_dvU);
int iem_soc_device(const iem_soc *q, double **d_csoc /* ncon: the accumulated residual */);
int iem_soc_state(iem_soc *q, iem_soc_state_t *out);      /* synchronises the stream: the one read-back */
/* HIP source of the five kernels and its cache key — for offline builds (no device needed; malloc'ed) */
int iem_soc_source(char **out_src, uint64_t *out_key);

/* ---- the feasibility restoration phase ---------------------------------------------------------------------------------------------
 * Step A-9 of Waechter and Biegler 2006 (Ipopt's section 3.3) on the device (csrc/iem_resto_device.h), as an object beside
 * iem_search: when the filter search of the ORIGINAL problem ends FAILED, the host enters the phase, iterates on the restoration
 * problem
 *     min  rho·sum(p + n) + zeta/2·|D_R (x − x_R)|²   s.t.  c(x) − s − p + n = 0 (inequality rows; c(x) − ceq − p + n = 0 on equality
 *     rows),  p, n >= 0,  the bounds of x and s
 * until the return test holds, and leaves.  With p, n eliminated the Newton system is the one iem_kkt_assemble_diag /
 * iem_kkt_solve_refined_diag solve: W is iem_jac_hess_coord with obj_weight = 0, r is iem_eval_residual with obj_weight = 0.  One
 * restoration iteration:
 *     iem_eval_residual(0);  iem_resto_error;  iem_jac_hess_coord(0);  iem_resto_terms;  iem_kkt_assemble_diag(dcon);  factor;
 *     iem_kkt_solve_refined_diag;  iem_resto_step;  iem_resto_merit(0);  iem_resto_begin;
 *     K × { iem_resto_trial, iem_cons, iem_resto_merit(1), iem_search_accept(inner, out, out + 1, mu, 1.0, alpha) };
 *     iem_resto_update;  iem_obj_device;  iem_cons;  iem_barrier_merit;  iem_resto_check
 * The host keeps the restoration problem's mu rule (iem_search_reset(inner) when mu changes) — or hands it to the iem_rmu object below,
 * which also binds these calls to a block on the device (iem_resto_bind_mu) —, the delta_w retry and one status read (iem_resto_state).
 * Notation: gaps, flags, sl, su, ml, mu_u and the row-side sigs, gs are those of the barrier contract above;  inf_j = c_j − ceq_j on
 * an equality row, c_j − s_j on an inequality row;  rho is an option;  zeta is a host double of the caller (eta·sqrt(mu), eta = 1).
 * Every operation is rounded once, in the order written.  The object owns p, n, zp, zn, dp, dn, dzp, dzn, pt, nt, sR, ws (ncon each)
 * and xR, wx (nvar each) — ONE allocation in this order, zeroed at create — a block of 8 words (0 state (int64)  1 theta_start
 * 2 theta, 3 phi of the last check  4 the maximum of iem_resto_leave  5–7 zero) and an INNER iem_search on the same barrier object
 * with the options of the original one (iem_resto_search).
 * iem_resto_enter (two launches; the caller passes mu = max(mu, max |inf|), out[2] of iem_barrier_error):  xR = x,  wx_i = m·m with
 *     m = min(1, 1/|x_i|);  sR, ws likewise on inequality rows;  per row  h = (mu − rho·inf)/(2 rho),  n = h + sqrt(h·h +
 *     (mu·inf)/(2 rho)),  p = inf + n,  zp = mu/p,  zn = mu/n,  y_j = 0;  every present bound multiplier z = min(rho, z).  Then one
 *     workgroup of 64 adds ((1 − gamma_theta)·theta0, phi0 − gamma_phi·theta0) from words 3 and 2 of the ORIGINAL block to the
 *     ORIGINAL filter by the rule of iem_search_accept (dominated entries leave first, order kept, a full filter sets flag bit 1) and
 *     writes theta_start = theta0, NaN into words 2, 3 and state ACTIVE into the object's block.
 * iem_resto_terms:  variable:  zw = zeta·wx,  sigma = (sl + su) + zw,  gx = (mu_u − ml) + zw·(x − xR),  rhs = −(r + gx).  Row:
 *     rc = (inf − p) + n,  Dp = p/zp,  Dn = n/zn,  ep = (mu − p·(rho − y))/zp,  en = (mu − n·(rho + y))/zn,  t = (rc − ep) + en,
 *     D = Dp + Dn.  Equality row: dcon = D, rhs_y = −t.  Inequality row:  zs = zeta·ws,  sigs' = sigs + zs,  gsr = gs + zs·(s − sR),
 *     rs' = gsr − y,  inv = 1/sigs',  dcon = inv + D,  rhs_y = −(t + rs'·inv).
 * iem_resto_step:  ds = (dy − rs')/sigs';  dz*, dv* by the formulas of iem_barrier_step;  into the object  dp = ep + Dp·dy,
 *     dn = en − Dn·dy,  dzp = ((rho − y) − zp) − dy,  dzn = ((rho + y) − zn) + dy.  Step lengths as in iem_barrier_step (seed 1.0,
 *     integer minimum on bit patterns, a NaN direction or a candidate not > 0 gives +0.0), with the further candidates
 *     ((−tau)·p)/dp where dp < 0, ((−tau)·n)/dn where dn < 0 for alpha_primal and ((−tau)·zp)/dzp where dzp < 0, ((−tau)·zn)/dzn
 *     where dzn < 0 for alpha_dual.
 * iem_resto_merit(which): at (x, s, c) with (p, n) (which = 0), or at the trial point the caller passes with (pt, nt) (which = 1):
 *     S0 = sum_j (p + n),  S1 = sum_i wx·((x − xR)·(x − xR)) + sum_ineq ws·((s − sR)·(s − sR)),  theta_R = sum_j |(inf − p) + n|,
 *     L = sum log gap + sum_j log p + sum_j log n;  out[0] = rho·S0 + (0.5·zeta)·S1,  out[1] = theta_R,  out[2] = L.  A lane adds its
 *     entries in index order (per row: the slack's gaps, then p, then n); the totals are summed in the fixed order of the barrier
 *     sums.  iem_search_accept(inner, out, out + 1, mu, 1.0, alpha) IS the restoration's acceptance test.
 * iem_resto_begin: the slope  sum_i gx·dx + sum_ineq gsr·ds + sum_j ((rho − mu/p)·dp + (rho − mu/n)·dn)  and the INNER block word
 *     for word as iem_search_begin leaves it, with phi0 = merit0[0] − mu·merit0[2], theta0 = merit0[1], alpha_max = alpha[0].
 * iem_resto_trial: with the inner block's alpha  xt, st as iem_search_trial and  pt = p + alpha·dp,  nt = n + alpha·dn;  under FAILED
 *     / UNUSABLE it stores nothing.
 * iem_resto_update: the rules of iem_barrier_update (either step length +0.0: nothing moves), and  p += alpha_p·dp,
 *     n += alpha_p·dn,  zp, zn stepped by alpha_d and guarded against the new p, n.
 * iem_resto_error: the layout of iem_barrier_error:  [0] max |(r + zw·(x − xR)) − zL + zU| (NaN without r)  [1] max over rows of
 *     |(rho − y) − zp|, |(rho + y) − zn| and on inequality rows |(zs·(s − sR) − y) − vL + vU|  [2] max |rc|  [3] max |gap·z − mu|
 *     including p·zp, n·zn  [4] sum |y|  [5] sum of the multipliers including zp, zn  [6] theta_R  [7] L (the bits of
 *     iem_resto_merit(0)'s out[1], out[2]).  The scaled error applies with the counts (ncon, nz + 2 ncon).
 * iem_resto_check (one workgroup; d_f from iem_obj_device, d_merit from iem_barrier_merit at the new iterate, mu the ORIGINAL
 *     problem's):  theta = d_merit[0],  phi = d_f − mu·d_merit[1].  With state ACTIVE: both are stored in words 2, 3, and the state
 *     becomes RETURN iff theta, phi are finite, theta <= kappa_resto·theta_start, theta <= theta_max (word 6 of the ORIGINAL block)
 *     and no ORIGINAL filter entry dominates (theta, phi).  With any other state nothing is written.
 * iem_resto_leave (two launches): the integer maximum of the present bound multipliers; then y = 0, every present bound multiplier
 *     becomes 1.0 iff that maximum exceeds bound_mult_reset_threshold (or is a NaN), and state NONE.
 * Every call runs on the handle's stream, asynchronous, capturable; nothing allocates after create, nothing synchronises and nothing
 * is copied to the host, except by iem_resto_state.  IEM_E_ARG before any device work: null required pointers (the slack side may
 * be NULL without inequality rows), rho <= 0, kappa_resto outside (0, 1), mu < 0, zeta < 0, tau outside (0, 1], which outside
 * {0, 1}.  The object borrows the search object and through it the barrier object: destroy it before them.  Not here (Ipopt's alpha_min rule as
 * the trigger and the restoration's own mu on the device are the iem_rmu object below): a second-order correction of the restoration, a nested restoration,
 * sharded handles. */
typedef struct iem_resto iem_resto;
typedef struct {
  uint64_t struct_size;                 /* set by the CALLER to sizeof(iem_resto_opts_t) */
  double rho, kappa_resto, bound_mult_reset_threshold;
} iem_resto_opts_t;                     /* NULL = Ipopt's defaults: 1000, 0.9, 1000 */
typedef struct {
  uint64_t struct_size;                 /* set by the CALLER to sizeof(iem_resto_state_t): at most that many bytes are written */
  int64_t state;                        /* word 0 of the block */
  double theta_start, theta, phi;       /* words 1–3 */
} iem_resto_state_t;
enum { IEM_RESTO_NONE = 0, IEM_RESTO_ACTIVE = 1, IEM_RESTO_RETURN = 2 };
int iem_resto_create(iem_search *fs, const iem_resto_opts_t *opts, iem_resto **out);
int iem_resto_destroy(iem_resto *q);
int iem_resto_search(const iem_resto *q, iem_search **out_inner);      /* the inner search: owned by the object, never to be destroyed */
int iem_resto_enter(iem_resto *q, const double *d_x, const double *d_s, double *d_y, double *d_zL, double *d_zU, double *d_vL, double *d_vU,
                    const double *d_c, double mu);
int iem_resto_terms(iem_resto *q, const double *d_x, const double *d_s, const double *d_y, const double *d_zL, const double *d_zU, const double *d_vL,
                    const double *d_vU, const double *d_r, const double *d_c, double mu, double zeta, double *d_sigma, double *d_dcon, double *d_rhs);
int iem_resto_step(iem_resto *q, const double *d_x, const double *d_s, const double *d_y, const double *d_zL, const double *d_zU, const double *d_vL,
                   const double *d_vU, const double *d_sol, double mu, double tau, double zeta, double *d_ds, double *d_dzL, double *d_dzU,
                   double *d_dvL, double *d_dvU, double *d_alpha /* 2 */);
int iem_resto_merit(iem_resto *q, int which, const double *d_x, const double *d_s, const double *d_c, double zeta, double *d_out /* 3 */);
int iem_resto_begin(iem_resto *q, const double *d_x, const double *d_s, const double *d_sol, const double *d_ds, const double *d_merit0 /* 3 */,
                    const double *d_alpha /* 2 */, double mu, double zeta);
int iem_resto_trial(iem_resto *q, const double *d_x, const double *d_s, const double *d_sol, const double *d_ds, double *d_xt, double *d_st);
int iem_resto_update(iem_resto *q, double *d_x, double *d_s, double *d_y, double *d_zL, double *d_zU, double *d_vL, double *d_vU, const double *d_sol,
                     const double *d_ds, const double *d_dzL, const double *d_dzU, const double *d_dvL, const double *d_dvU, const double *d_alpha /* 2 */,
                     double mu, double kappa_sigma);
int iem_resto_error(iem_resto *q, const double *d_x, const double *d_s, const double *d_y, const double *d_zL, const double *d_zU, const double *d_vL,
                    const double *d_vU, const double *d_r /* may be NULL */, const double *d_c, double mu, double zeta, double *d_out /* 8 */);
int iem_resto_check(iem_resto *q, const double *d_f, const double *d_merit /* 2 */, double mu);
int iem_resto_leave(iem_resto *q, double *d_y, double *d_zL, double *d_zU, double *d_vL, double *d_vU);
int iem_resto_device(const iem_resto *q, double **d_p, double **d_n, double **d_zp, double **d_zn, void **d_block);      /* any may be NULL */
int iem_resto_state(iem_resto *q, iem_resto_state_t *out);      /* synchronises the stream: the one read-back */
/* HIP source of the twelve kernels and its cache key — for offline builds (no device needed; malloc'ed) */
int iem_resto_source(char **out_src, uint64_t *out_key);

/* ---- the barrier parameter ---------------------------------------------------------------------------------------------------------
 * mu, tau and the stopping test of a monotone (Fiacco–McCormick) interior-point method on the device (csrc/iem_mu_device.h), as an
 * object beside iem_barrier: the error terms with what the rule needs of the complementarity products (iem_mu_error), and the rule
 * (iem_mu_update).  The values live in a block on the device that the kernels of iem_barrier, iem_search and iem_soc read once their
 * object is BOUND to it (iem_*_bind_mu below), so one captured iteration
 *     iem_eval_residual;  iem_mu_error;  iem_mu_update(fs);  iem_barrier_terms;  ...;  iem_search_begin;  rungs;  iem_barrier_update
 * replays across a change of mu, and the host reads one struct per iteration (iem_mu_state).
 *
 * THE BLOCK: sixteen 8-byte words on the device (iem_mu_device gives the pointer):
 *     0 mu      1 tau = max(tau_min, 1 − mu)      2 zeta = sqrt(mu) (what a bound iem_resto reads: iem_resto_bind_mu)      3 E(0)
 *     4 E(mu) at the mu the call leaves behind      5 e_d      6 e_p      7 e_c(0)
 *     8 status (int64): 0 ITERATING, 1 CONVERGED, 2 UNUSABLE      9 flags (int64): bit 0 = mu changed in the last update
 *     10 decreases so far (int64)      11 updates so far (int64)      12–15 zero
 * iem_mu_create writes words 0–2 from mu_init and zeroes the rest.  iem_mu_reset (one launch of one workgroup, asynchronous) writes
 *     words 0–2 from mu0 and zeroes words 8–11; words 3–7 stay.
 * iem_mu_error: ONE launch on the barrier object's grid behind one 96-byte device-to-device copy (the seed of the extremes), twelve
 *     words.  [0]–[7] are bit for bit what iem_barrier_error(mu = 0) writes on the same inputs (the same per-lane order, the same
 *     fixed-order totals; the partial sums are the object's own).  With p = gap·z over the present bounds, each product rounded once:
 *     [8] the minimum of the p that are >= +0.0 (an integer minimum on bit patterns seeded with +inf; a negative product, −0.0 or a
 *     NaN does not enter)  [9] the sum of all p, the lane's entries in index order, the totals in the fixed order of the barrier
 *     sums  [10] the count of the p that did not enter [8], as a double (exact)  [11] +0.0.  d_r is required: no NaN form.
 * iem_mu_update: ONE workgroup of 64 threads, one thread decides, each operation rounded once, every max / min propagating a NaN.
 *     With w the twelve words, m = ncon and nz of iem_barrier_info:
 *         sd = max(s_max, (w4 + w5)/max(1, m + nz))/s_max      sc = max(s_max, w5/max(1, nz))/s_max
 *         e_d = max(w0, w1)/sd      e_p = m ? w2 : 0      e_c(mu) = nz ? max(w3 − mu, mu − w8)/sc : 0      E(mu) = max(max(e_d, e_p), e_c(mu))
 *     (rounding is monotone, so max(w3 − mu, mu − w8) carries the bits of max |p − mu|: word 3 of iem_barrier_error at that mu).
 *     w10 != 0 or E(0) a NaN: status UNUSABLE, mu, tau, zeta stay.  Else E(0) <= tol: CONVERGED, mu stays.  Else ITERATING and
 *         k = 0;  while mu > mu_floor and E(mu) <= kappa_eps·mu and k < 64:  mu = max(mu_floor, min(kappa_mu·mu, mu·sqrt(mu)));  k += 1
 *     (sqrt correctly rounded; the exponent 1.5 is Ipopt's mu_superlinear_decrease_power and not an option).  k > 0: words 0–2 are
 *     rewritten, flag bit 0 is set, word 10 grows by k, and words 11 and 12 of fs's control block are zeroed when fs is given —
 *     the 16 bytes of iem_search_reset.  k = 0: flag bit 0 is cleared, fs is untouched.  Word 11 grows by 1 and words 3–7 are
 *     stored either way.
 * BINDING: iem_barrier_bind_mu / iem_search_bind_mu / iem_soc_bind_mu (p = NULL unbinds; no launch — the first iem_barrier_bind_mu of a handle
 *     loads the bound variant of the barrier code object, so bind outside a capture).  While an
 *     object is bound, barrier_terms / step / update / error, search_begin / accept and soc_rhs / accept read mu from word 0 (and
 *     barrier_step tau from word 1) where they read their argument before, once, at the same place: the host's mu and tau arguments
 *     and their range checks are ignored.  Unbound, every call writes the bits it wrote before.  Binding is per object: the inner
 *     search of an iem_resto borrows the same barrier object and keeps the restoration problem's own mu — bind the barrier object
 *     only while the original problem iterates.  iem_resto_* reads a block only once bound to an iem_rmu (iem_resto_bind_mu).
 * Every call runs on the handle's stream, asynchronous, capturable; nothing allocates after create, nothing synchronises and nothing
 * is copied to the host, except by iem_mu_state.  IEM_E_ARG before any device work: null required pointers (the slack side may be
 * NULL without inequality rows), mu_init <= 0, kappa_mu or tau_min outside (0, 1), kappa_eps <= 0, tol <= 0, mu_floor < 0,
 * s_max <= 0, any option not finite, mu0 <= 0 or not finite, an fs or a bind across two barrier objects.  The object borrows the
 * barrier object; a bound object borrows the block: unbind (or destroy the bound objects) before iem_mu_destroy.  Not here: the
 * delta_w / inertia retry, sharded handles.  The adaptive rules that words 8 and 9 of iem_mu_error
 * serve (probing, LOQO) are the iem_amu object below, the quality-function oracle the iem_qf object below it, Mehrotra's corrector
 * the iem_mpc object below that. */
typedef struct iem_mu iem_mu;
typedef struct {
  uint64_t struct_size;                 /* set by the CALLER to sizeof(iem_mu_opts_t) */
  double mu_init, kappa_eps, kappa_mu, tau_min, tol, mu_floor, s_max;
} iem_mu_opts_t;                        /* NULL = Ipopt's defaults: 0.1, 10, 0.2, 0.99, 1e-8, 0 (= max(1e-11, tol/10)), 100 */
typedef struct {
  uint64_t struct_size;                 /* set by the CALLER to sizeof(iem_mu_state_t): at most that many bytes are written */
  double mu, tau, zeta, e0, e_mu, e_d, e_p, e_c0;      /* words 0–7 of the block */
  int64_t status, flags, decreases, updates;           /* words 8–11 */
} iem_mu_state_t;
enum { IEM_MU_ITERATING = 0, IEM_MU_CONVERGED = 1, IEM_MU_UNUSABLE = 2 };
int iem_mu_create(iem_barrier *b, const iem_mu_opts_t *opts, iem_mu **out);
int iem_mu_destroy(iem_mu *p);
int iem_mu_reset(iem_mu *p, double mu0);
int iem_mu_error(iem_mu *p, const double *d_x, const double *d_s, const double *d_y, const double *d_zL, const double *d_zU, const double *d_vL,
                 const double *d_vU, const double *d_r, const double *d_c, double *d_out /* 12 */);
int iem_mu_update(iem_mu *p, const double *d_out12, iem_search *fs /* may be NULL */);
int iem_mu_device(const iem_mu *p, double **d_block);
int iem_mu_state(iem_mu *p, iem_mu_state_t *out);      /* synchronises the stream: the one read-back */
int iem_barrier_bind_mu(iem_barrier *b, const iem_mu *p /* NULL unbinds */);
int iem_search_bind_mu(iem_search *fs, const iem_mu *p /* NULL unbinds */);
int iem_soc_bind_mu(iem_soc *q, const iem_mu *p /* NULL unbinds */);
/* HIP source of the three kernels and its cache key — for offline builds (no device needed; malloc'ed) */
int iem_mu_source(char **out_src, uint64_t *out_key);
/* ... and of the BOUND variant of the barrier code object: the text of iem_barrier_source with BarrierArgs one pointer longer and the
 * reads of mu and tau taken from the block; iem_barrier_bind_mu loads it.  iem_barrier_source, its key and the unbound calls are unchanged */
int iem_barrier_mu_source(char **out_src, uint64_t *out_key);

/* ---- the adaptive barrier parameter --------------------------------------------------------------------------------------------------
 * Ipopt's `mu_strategy = adaptive` with the kkt-error globalisation on the device (csrc/iem_amu_device.h), as an object created ON an
 * iem_mu: it drives that object's block, so every kernel bound through iem_*_bind_mu keeps reading word 0 (mu) and word 1 (tau) of the
 * same block, and one captured iteration still replays across every change of mu.  Per iteration the host calls EITHER iem_mu_update
 * OR iem_amu_update on the block.  kappa_eps, kappa_mu, tau_min, tol, mu_floor and s_max are those of the iem_mu object.
 *
 * THE OWN BLOCK: sixteen 8-byte words on the device (iem_amu_device gives the pointer; iem_amu_state_t mirrors words 0–13):
 *     0 mode (int64): 0 FREE, 1 FIXED      1 mu_max (+0.0: unset)      2 reference count (int64)      3–6 references, oldest first
 *     7 the oracle's mu before clamping      8 sigma      9 avg      10 m_aff (+0.0 for LOQO)
 *     11 switches to FIXED (int64)      12 switches to FREE (int64)      13 oracle (int64): 0 probing, 1 LOQO      14–15 zero
 * iem_amu_create zeroes it but for word 13.  iem_amu_reset (one launch of one workgroup, asynchronous) does the same: mode FREE, the
 *     ring empty, mu_max unset, words 7–12 zero.  The iem_mu block has its own iem_mu_reset.
 * iem_amu_probe: the complementarity that the affine-scaling step would leave behind.  ONE launch on the barrier object's grid, the
 *     entry order and flags of iem_mu_error, no seed (the last workgroup writes all four words), no host memset, no synchronisation,
 *     capturable.  With ap = alpha_aff[0], ad = alpha_aff[1] read once, d = dx (sol[i]) on variables and ds on rows, per PRESENT bound,
 *     each operation rounded once, in this order:
 *         t = ap·d      g = gap + t (lower bound; gap = x − xl or s − rl)      g = gap − t (upper bound; gap = xu − x or ru − s)
 *         u = ad·dz      w = z + u      p = g·w
 *     [0] the sum of all p — a lane adds its entries in index order (lower before upper), the workgroups park, the last arrival totals
 *     in the fixed order of the barrier sums: with all directions +0.0 and alpha_aff = (1, 1) these are the bits of word 9 of
 *     iem_mu_error on the same state  [1] the count of the p that are NaN, as a double (exact)  [2] ap  [3] ad.  Absent bounds and
 *     equality rows are never read (neither state nor direction); y and dy are not read at all.
 *     THE AFFINE DIRECTION comes from existing calls: sigma and dcon of iem_barrier_terms do not depend on mu, so
 *         iem_barrier_terms(mu = 0) -> rhs_aff;  iem_kkt_solve_refined_diag on the iteration's factors;  iem_barrier_step(mu = 0, tau = 1)
 *     with the barrier object UNBOUND around them (iem_barrier_bind_mu(b, NULL) ... iem_barrier_bind_mu(b, p): no launch after the
 *     first bind; a capture bakes each node's variant and pointers).
 * iem_amu_update: ONE workgroup of 64 threads, one thread decides, each operation rounded once, every max / min propagating a NaN.
 *     With w the twelve words of iem_mu_error and q the four of iem_amu_probe (required for the probing oracle, NULL for LOQO), sd,
 *     sc, e_d, e_p, e_c(mu), E(mu) are iem_mu_update's expressions.  Words 3–7, the status and updates += 1 of the iem_mu block are
 *     stored as iem_mu_update stores them (word 4 at the mu the call leaves behind).
 *     UNUSABLE: w10 != 0, E(0) a NaN, or (probing) q1 != 0, q2 or q3 the bits of +0.0 (an unusable affine step) — mu, tau, zeta and
 *         the own block stay.  Else CONVERGED: E(0) <= tol — mu and the own block stay.  Else ITERATING:
 *     nz == 0: mu = mu_min, nothing else.  Otherwise
 *         avg = w9/nz (word 9);  mu_max = mu_max_fact·avg if word 1 is +0.0 (kept until iem_amu_reset)
 *         progress = n < refs_max  ||  E(0) <= red_fact·max(references)          remember(E0): append; at refs_max drop the oldest first
 *         mode FIXED:  progress ? (mode <- FREE, word 12 += 1, remember(E0))
 *                               : the loop of iem_mu_update — the same condition, expression and cap of 64; decreases += k
 *         mode FREE:   progress && !force_fixed ? remember(E0)
 *                               : (mode <- FIXED, word 11 += 1, mu = min(max(init_factor·avg, mu_min), mu_max))
 *         then, if the mode is FREE: the oracle, words 7, 8, 10, and mu = min(max(word 7, mu_min), mu_max)
 *             probing:  m_aff = q0/nz;  r = m_aff/avg;  sigma = min((r·r)·r, sigma_max);  word 7 = sigma·avg
 *             LOQO:     xi = w8/avg;  f = (0.05·(1 − xi))/xi;  c = min(f, 2.0);  sigma = 0.1·((c·c)·c);  word 7 = sigma·avg
 *     (no pow: three multiplications).  If the BITS of mu changed: words 0–2 are rewritten (tau = max(tau_min, 1 − mu), zeta =
 *     sqrt(mu) correctly rounded), flag bit 0 is set, and words 11 and 12 of fs's control block are zeroed when fs is given.
 *     Otherwise flag bit 0 is cleared and fs is untouched.  force_fixed is the host's verdict on the last step (a failed search, a
 *     tiny step): Ipopt's switch to the monotone mode.
 * iem_amu_state: the one read-back — both blocks behind ONE synchronisation.
 * Every call runs on the handle's stream, asynchronous, capturable; nothing allocates after create.  IEM_E_ARG before any device
 * work: null required pointers (the slack side may be NULL without inequality rows), a probing object updated without q, an fs of
 * another barrier object, oracle not 0 or 1, sigma_max, mu_min, mu_max_fact or init_factor <= 0, red_fact outside (0, 1), refs_max
 * outside 1..4, any option not finite.  The object borrows the iem_mu object: destroy it first.  Ipopt's quality-function oracle
 * (oracle = 2 here is refused) is the iem_qf object below, Mehrotra's corrector the iem_mpc object below that.  Not here: the
 * obj-constr-filter globalisation, sharded handles, the delta_w / inertia retry (the host's). */
typedef struct iem_amu iem_amu;
typedef struct {
  uint64_t struct_size;                 /* set by the CALLER to sizeof(iem_amu_opts_t) */
  int64_t oracle;                       /* IEM_AMU_PROBING / IEM_AMU_LOQO */
  double sigma_max, mu_min, mu_max_fact, init_factor, red_fact;
  int64_t refs_max;                     /* 1..4 */
} iem_amu_opts_t;                       /* NULL = probing, 100, 1e-11, 1e3, 0.8, 0.9999, 4 */
typedef struct {
  uint64_t struct_size;                 /* set by the CALLER to sizeof(iem_amu_state_t): at most that many bytes are written */
  int64_t mode;                         /* word 0 */
  double mu_max;                        /* word 1 */
  int64_t refs_count;                   /* word 2 */
  double refs[4];                       /* words 3–6 */
  double mu_oracle, sigma, avg, m_aff;  /* words 7–10 */
  int64_t to_fixed, to_free, oracle;    /* words 11–13 */
} iem_amu_state_t;
enum { IEM_AMU_FREE = 0, IEM_AMU_FIXED = 1 };
enum { IEM_AMU_PROBING = 0, IEM_AMU_LOQO = 1 };
int iem_amu_create(iem_mu *p, const iem_amu_opts_t *opts, iem_amu **out);
int iem_amu_destroy(iem_amu *a);
int iem_amu_reset(iem_amu *a);
int iem_amu_probe(iem_amu *a, const double *d_x, const double *d_s, const double *d_zL, const double *d_zU, const double *d_vL, const double *d_vU,
                  const double *d_sol_aff, const double *d_ds_aff, const double *d_dzL_aff, const double *d_dzU_aff, const double *d_dvL_aff,
                  const double *d_dvU_aff, const double *d_alpha_aff /* 2 */, double *d_out /* 4 */);
int iem_amu_update(iem_amu *a, const double *d_out12 /* of iem_mu_error */, const double *d_probe4 /* NULL for LOQO */, int force_fixed,
                   iem_search *fs /* may be NULL */);
int iem_amu_device(const iem_amu *a, double **d_block);
int iem_amu_state(iem_amu *a, iem_mu_state_t *mu_out, iem_amu_state_t *out);      /* synchronises the stream: the one read-back */
/* HIP source of the three kernels and its cache key — for offline builds (no device needed; malloc'ed) */
int iem_amu_source(char **out_src, uint64_t *out_key);

/* ---- the quality-function oracle -------------------------------------------------------------------------------------------------------
 * Ipopt's `mu_oracle = quality-function` (its default for mu_strategy = adaptive; QualityFunctionMuOracle with the 2-norm squared,
 * no centrality and no balancing term; MadNLP's adaptive update has the same one) on the device (csrc/iem_qf_device.h), as an object
 * created ON an iem_amu: it reads that object's block and the iem_mu block under it, and iem_qf_update goes in the place of
 * iem_amu_update.  sigma_max defaults to the iem_amu object's; mu_min, mu_max_fact, init_factor, red_fact, refs_max are that
 * object's, kappa_eps, kappa_mu, tau_min, tol, mu_floor and s_max those of the iem_mu object.  The iem_amu object's oracle option
 * is not consulted.
 *
 * THE DIRECTION for a candidate sigma comes from existing calls.  The Newton direction is affine in mu for fixed factors, so with the
 * barrier object UNBOUND (iem_barrier_bind_mu(b, NULL)):
 *         iem_barrier_terms(mu = 0) and iem_barrier_terms(mu = mu_ref) -> two right-hand-side columns (sigma, dcon do not depend on mu);
 *         one assemble + factor (the host's delta_w retry);  ONE iem_kkt_solve_refined_diag(nrhs = 2);
 *         iem_barrier_step(mu = 0, tau = 1) -> d0,  iem_barrier_step(mu = mu_ref, tau = 1) -> d1 (their alphas are ignored)
 *     and for every component the oracle reads (dx = sol[i], ds, dzL, dzU, dvL, dvU; never dy), each operation rounded once:
 *         t = sigma·avg;  t = t/mu_ref          (once per thread)          e = d1 − d0;  u = t·e;  d = d0 + u
 *     ONE device function forms d for both grid kernels.  With d1 = d0 the direction is d0 bit for bit (but −0.0 becomes +0.0).
 *
 * THE OWN BLOCK: thirty-two 8-byte words on the device (iem_qf_device gives the pointer; iem_qf_state_t mirrors words 0–26):
 *     0 status (int64): 0 IDLE, 1 SECTION, 2 DONE, 3 UNUSABLE      1 phase (int64): which evaluation is next — 0 the first sigma,
 *     1 the second, 2 / 3 the left / right interior point of the first bracket, 4 / 5 a new left / right interior point
 *     2 section steps taken (int64)      3 evaluations (int64)      4 sigma: the trial the next alpha / value pair evaluates
 *     5, 6 the alpha slots (alpha_primal, alpha_dual as bit patterns)      7 D2      8 P2      9 avg      10 lo      11 hi
 *     12, 13 the bracket [a, b]      14, 15 its interior points c < d      16, 17 q(c), q(d)
 *     18 the evaluated sigma of least q      19 that q      20 q at the first sigma
 *     21–25 the last evaluation: q, C2, the count of NaN products, alpha_primal, alpha_dual      26 the first sigma      27–31 zero
 * iem_qf_create zeroes it (IDLE); iem_qf_reset (one launch of one workgroup, asynchronous) does the same.
 * iem_qf_begin: ONE launch on the barrier object's grid, the entry order and flags of iem_mu_error, no seed, capturable.  Two sums,
 *     a lane adding its entries in index order, the workgroups parking, the last arrival totalling in the fixed order of the
 *     barrier sums:   D2 = sum over variables of t·t, t = r − zL + zU, and over inequality rows of t·t, t = −y − vL + vU;
 *     P2 = sum over rows of inf·inf, inf = c − ceq (equality) or c − s — the residual expressions of iem_barrier_error, in its
 *     order (t = r; t = t − zL where the lower bound is present; t = t + zU where the upper one is).  The last arrival then zeroes
 *     the block, stores D2 and P2 and, with w the twelve words of iem_mu_error and every max / min propagating a NaN,
 *         nz == 0:  status DONE, nothing else.  Otherwise
 *         avg = w9/nz;  mu_max = word 1 of the iem_amu block, or mu_max_fact·avg while that word is +0.0 (the word is not written)
 *         lo = max(sigma_min, mu_min/avg);  hi = max(lo, min(sigma_max, mu_max/avg));  sigma = min(max(1, lo), hi)
 *         the alpha slots = the bits of 1.0;  phase 0;  status SECTION.
 * iem_qf_alpha: ONE launch on the same grid: the fraction-to-the-boundary step lengths of d(sigma) — the candidates
 *     (−tau·gap)/d, (tau·gap)/d, (−tau·z)/dz and the unusable-value rules of iem_barrier_step (a candidate that is not > 0 counts
 *     as +0.0; a NaN in dx or in the ds of an inequality row makes alpha_primal +0.0 whatever the bounds, a NaN in a multiplier's
 *     direction at a present bound makes alpha_dual +0.0) — except that dy is not read and tau is word 1 of the iem_mu block.
 *     Integer minima on the bit patterns into slots 5 and 6, at most one atomic per workgroup and slot.
 * iem_qf_value: ONE launch on the same grid.  With ap, ad the two slots read once, per PRESENT bound in the operation order of
 *     iem_amu_probe:   t = ap·d;  g = gap + t (lower) or gap − t (upper);  u = ad·dz;  w = z + u;  p = g·w;   the columns
 *     C2 = sum of p·p and the count of the p that are NaN are parked and totalled as above.  The last arrival forms
 *         q = +inf  if ap or ad carries the bits of +0.0 or a product was a NaN; otherwise
 *         ud = 1 − ad;  up = 1 − ap;  td = ((ud·ud)·D2)/n_d;  tp = ((up·up)·P2)/n_p;  tc = C2/nz;  q = (td + tp) + tc
 *     with n_d = nvar + inequality rows, n_p = ncon, a term whose count is 0 being +0.0, and a NaN q counting as +inf; then it
 *     takes ONE step of the section below, writes the next trial sigma into word 4 and re-seeds the two slots with the bits of 1.0.
 * THE SECTION, word for word (g = 0.6180339887498949, tol = section_sigma_tol, every comparison on q with NaN already +inf):
 *     every evaluation:  evaluations += 1;  words 21–25;  if it is the first or q < word 19: words 18, 19 = sigma, q (the first of
 *         equal values stays)
 *     phase 0:  word 20 = q;  sigma <- max(lo, sigma·(1 − 1e-2));  phase 1
 *     phase 1:  [a, b] = [lo, sigma] if q <= word 20, else [first sigma, hi];  w = b − a;  if w <= tol·b: FINISH;  else
 *               gw = g·w;  c = b − gw;  d = a + gw;  sigma <- c;  phase 2
 *     phase 2:  q(c) = q;  sigma <- d;  phase 3
 *     phase 3 or 5:  q(d) = q;  STEP            phase 4:  q(c) = q;  STEP
 *     STEP:  if steps == max_section_steps: FINISH;  else
 *               q(c) <= q(d):  b = d;  d = c;  q(d) = q(c);  gw = g·(b − a);  c = b − gw;  sigma <- c;  phase 4
 *               otherwise:     a = c;  c = d;  q(c) = q(d);  gw = g·(b − a);  d = a + gw;  sigma <- d;  phase 5
 *            steps += 1;  if b − a <= tol·b: FINISH (the new point is not evaluated)
 *     FINISH:  status = UNUSABLE if word 19 is +inf (every q was), else DONE;  word 4 stays.
 *     So there is one new evaluation per step, at most max_section_steps + 4 evaluations in all, and lo == hi finishes after two.
 *     With a status other than SECTION, iem_qf_alpha and iem_qf_value return before their first store: the host issues
 *     max_section_steps + 4 alpha / value pairs with no decision in between, and a captured sequence is valid at every state.
 * iem_qf_update: ONE workgroup of 64 threads, one thread decides: iem_amu_update's rule word for word on the same two blocks —
 *     the stopping test, the ring of references, the free / fixed modes, the monotone loop, fs's filter emptied exactly when the
 *     bits of mu changed.  Only the free-mode oracle differs: sigma (word 8 of the iem_amu block) = word 18, word 7 = sigma·avg,
 *     word 10 = word 19; and UNUSABLE has one more condition: a section whose status is not DONE.
 * iem_qf_state: the one read-back — the iem_mu block, the iem_amu block and the own block behind ONE synchronisation.
 * Every call runs on the handle's stream, asynchronous, capturable; nothing allocates after create.  No float atomic, no cooperative
 * launch, no grid-wide wait: every dependence between workgroups is a launch boundary.  IEM_E_ARG before any device work: null
 * required pointers (the slack side may be NULL without inequality rows), an fs of another barrier object, mu_ref, sigma_min or
 * section_sigma_tol <= 0, sigma_max < 0 (0: the iem_amu object's), max_section_steps outside 1..16, any option not finite.  The
 * object borrows the iem_amu object: destroy it first.  Mehrotra's corrector is the iem_mpc object below.  Not here: Ipopt's other
 * norm types, the centrality and balancing terms, the obj-constr-filter globalisation, sharded handles, the
 * delta_w / inertia retry. */
typedef struct iem_qf iem_qf;
typedef struct {
  uint64_t struct_size;                 /* set by the CALLER to sizeof(iem_qf_opts_t) */
  double mu_ref, sigma_min, sigma_max, section_sigma_tol;
  int64_t max_section_steps;            /* 1..16 */
} iem_qf_opts_t;                        /* NULL = 1.0, 1e-6, 0 (= the iem_amu object's sigma_max), 1e-2, 8 */
typedef struct {
  uint64_t struct_size;                 /* set by the CALLER to sizeof(iem_qf_state_t): at most that many bytes are written */
  int64_t status, phase, steps, evaluations;      /* words 0–3 */
  double sigma_trial;                   /* word 4 */
  double alpha_slots[2];                /* words 5, 6 */
  double d2, p2, avg, lo, hi;           /* words 7–11 */
  double a, b, c, d, qc, qd;            /* words 12–17 */
  double sigma, q, q_first;             /* words 18–20: the result, its q, q at the first sigma */
  double q_last, c2_last, nan_last, alpha_p_last, alpha_d_last;      /* words 21–25 */
  double sigma_first;                   /* word 26 */
} iem_qf_state_t;
enum { IEM_QF_IDLE = 0, IEM_QF_SECTION = 1, IEM_QF_DONE = 2, IEM_QF_UNUSABLE = 3 };
int iem_qf_create(iem_amu *a, const iem_qf_opts_t *opts, iem_qf **out);
int iem_qf_destroy(iem_qf *q);
int iem_qf_reset(iem_qf *q);
int iem_qf_begin(iem_qf *q, const double *d_x, const double *d_s, const double *d_y, const double *d_zL, const double *d_zU, const double *d_vL, const double *d_vU,
                 const double *d_r, const double *d_c, const double *d_out12 /* of iem_mu_error */);
int iem_qf_alpha(iem_qf *q, const double *d_x, const double *d_s, const double *d_zL, const double *d_zU, const double *d_vL, const double *d_vU,
                 const double *d_sol0, const double *d_ds0, const double *d_dzL0, const double *d_dzU0, const double *d_dvL0, const double *d_dvU0,
                 const double *d_sol1, const double *d_ds1, const double *d_dzL1, const double *d_dzU1, const double *d_dvL1, const double *d_dvU1);
int iem_qf_value(iem_qf *q, const double *d_x, const double *d_s, const double *d_zL, const double *d_zU, const double *d_vL, const double *d_vU,
                 const double *d_sol0, const double *d_ds0, const double *d_dzL0, const double *d_dzU0, const double *d_dvL0, const double *d_dvU0,
                 const double *d_sol1, const double *d_ds1, const double *d_dzL1, const double *d_dzU1, const double *d_dvL1, const double *d_dvU1);
int iem_qf_update(iem_qf *q, const double *d_out12 /* of iem_mu_error */, int force_fixed, iem_search *fs /* may be NULL */);
int iem_qf_device(const iem_qf *q, double **d_block);
int iem_qf_state(iem_qf *q, iem_mu_state_t *mu_out, iem_amu_state_t *amu_out, iem_qf_state_t *out);      /* synchronises the stream: the one read-back */
/* HIP source of the five kernels and its cache key — for offline builds (no device needed; malloc'ed) */
int iem_qf_source(char **out_src, uint64_t *out_key);

/* ---- Mehrotra's corrector --------------------------------------------------------------------------------------------------------------
 * The second-order term of the complementarity equations on the right-hand side (Ipopt's `mehrotra_algorithm = yes`, every LP / QP
 * interior-point code) on the device (csrc/iem_mpc_device.h), as an object created ON an iem_amu: it borrows that object, the iem_mu
 * block under it and the barrier object's bounds, flags and grid.  The affine-scaling direction (sol_aff, ds_aff, dzL_aff, dzU_aff,
 * dvL_aff, dvU_aff: what iem_amu_probe is handed; with iem_qf its d0) carries the term dgap_aff·dz_aff; the corrected direction solves
 * the Newton system whose complementarity rows have the target mu − dgap_aff·dz_aff in the place of mu.  It costs one more column of
 * the iteration's refined solve, no factorisation and no host decision.  The calls run AFTER the rule's update (iem_amu_update /
 * iem_qf_update), at the new mu, with the objects bound again.
 *
 * Entry order, flags (fx / fc) and what is never read are those of iem_barrier_terms / iem_barrier_step: one thread takes the entries
 * i, i + stride, ... of [0, nvar + ncon); nothing is read where no bound is present, nor on equality rows of the slack side; dy_aff
 * (sol_aff past nvar) is never read.  Each operation is rounded once, in the order written here.  With d_aff = sol_aff[i] on variables
 * and ds_aff[j] on inequality rows, per PRESENT bound:
 *         lower bound:  e = d_aff·dz_aff;  m = mu − e          upper bound:  e = d_aff·dz_aff;  m = mu + e      (its gap moves by −d)
 * iem_mpc_terms: ONE launch on the barrier object's grid.  Two columns, d_rhs2 + u·ld (ld >= nvar + ncon; the layout of
 *     iem_kkt_solve_refined_diag).  Column 0 is bit for bit the rhs of iem_barrier_terms at that mu.  Column 1 is the same expressions
 *     with m in the place of mu:   ml = m/gap (lower; else +0.0);  mu_u = m/gap (upper; else +0.0);  variables: gb = mu_u − ml;
 *     rhs = −(r + gb);  inequality rows: sl = vL/gap, su = vU/gap, sigs = sl + su;  gs = mu_u − ml;  rs = gs − y;  inv = 1.0/sigs;
 *     rhs = −((c − s) + rs·inv);  equality rows: −(c − ceq) in both columns.  sigma and dcon are NOT written: they do not depend on mu
 *     and exist from the affine iem_barrier_terms call.
 * iem_mpc_step: ONE launch on the same grid behind one 16-byte device-to-device copy (the step lengths' seed, the bits of 1.0), on
 *     the CORRECTED solution (column 1 of the solve).  iem_barrier_step word for word with m in the place of mu:
 *         variables:  dzL = (m/gap − zL) − (zL/gap)·dx;  dzU = (m/gap − zU) + (zU/gap)·dx      (absent bound: +0.0)
 *         rows:  ml = m/gap, mu_u = m/gap;  gs = mu_u − ml;  rs = gs − y;  ds = (dy − rs)/sigs;  dvL = (ml − vL) − sl·ds;
 *                dvU = (mu_u − vU) + su·ds
 *     and its candidates (−tau·gap)/d, (tau·gap)/d, (−tau·z)/dz, its NaN rules (a NaN in dx, dy or the ds of an inequality row makes
 *     alpha_primal +0.0 whatever the bounds, a NaN in a multiplier's direction at a present bound makes alpha_dual +0.0; a candidate
 *     that is not > 0 counts as +0.0) and its integer minima on bit patterns, at most one atomic per workgroup and slot.  Column 0 of
 *     the solve goes through iem_barrier_step, unchanged.
 * THE SAFEGUARD'S MEASUREMENT is iem_amu_probe on the corrected direction at alpha_c: four words q_c.  A launch of its own because it
 *     needs alpha_c: every dependence between workgroups is a launch boundary.
 * iem_mpc_select: ONE launch on the same grid.  Every thread reads q_c, the two words of alpha_c and word 9 (avg) of the iem_amu block
 *     — none of which the launch writes — and decides the same way.  With nz of iem_barrier_info:
 *         predicted = nz ? q_c[0]/nz : +0.0;   bound = red_fact·avg
 *         TAKEN  iff  nz != 0  and  q_c[1] == 0  and  neither word of alpha_c is the bits of +0.0  and  predicted <= bound
 *     (a NaN compares false; red_fact = 1.0 is Ipopt's corrector_compl_avrg_red_fact).  Taken, the corrected direction is copied
 *     over the first-order one, exactly the entries iem_soc_select copies — sol: nvar + ncon; dzL, dzU: nvar; ds, dvL, dvU:
 *     inequality rows only — and d_alpha takes the two words of alpha_c.  Refused, the call returns before its first store to a
 *     direction.  iem_search_begin, the rungs, iem_soc_* and iem_barrier_update then run on the first-order buffers as before.
 * THE OWN BLOCK: sixteen 8-byte words on the device (iem_mpc_device gives the pointer; iem_mpc_state_t mirrors words 0–6), written by
 *     one thread of workgroup 0 of iem_mpc_select:
 *     0 the decision of this call (int64): 1 taken, 0 refused      1 correctors taken so far (int64)      2 refused so far (int64)
 *     3 predicted      4 avg      5, 6 alpha_c (alpha_primal, alpha_dual)      7–15 zero
 *     iem_mpc_create zeroes it; iem_mpc_reset (one launch of one workgroup, asynchronous) does the same.
 * iem_mpc_bind_mu(q, p): bound, mpc_terms / mpc_step read mu and tau from words 0 and 1 of the iem_mu block and ignore their
 *     arguments and the range checks; p = NULL unbinds: they take the host's mu >= 0 and tau in (0, 1].  No launch, one code object.
 * iem_mpc_state: the one read-back (one synchronisation).
 * Every call runs on the handle's stream, asynchronous, capturable; nothing allocates after create.  No float atomic, no cooperative
 * launch.  IEM_E_ARG before any device work: null required pointers (the slack side may be NULL without inequality rows),
 * ld < nvar + ncon, red_fact not finite or <= 0, an iem_mu passed to iem_mpc_bind_mu that is not the object's own, unbound mu < 0 or
 * tau outside (0, 1], d_alpha == d_alpha_c.  The object borrows the iem_amu object: destroy it first.  Not here: Ipopt's
 * accept_every_trial_step and the other options mehrotra_algorithm implies, Gondzio's multiple centrality correctors, a corrector
 * inside iem_resto, sharded handles, the delta_w / inertia retry.  iem_soc_rhs is unchanged: the second-order correction's own
 * right-hand side keeps the target mu. */
typedef struct iem_mpc iem_mpc;
typedef struct {
  uint64_t struct_size;                 /* set by the CALLER to sizeof(iem_mpc_opts_t) */
  double red_fact;
} iem_mpc_opts_t;                       /* NULL = 1.0 */
typedef struct {
  uint64_t struct_size;                 /* set by the CALLER to sizeof(iem_mpc_state_t): at most that many bytes are written */
  int64_t taken, n_taken, n_refused;    /* words 0–2 */
  double predicted, avg;                /* words 3, 4 */
  double alpha_c[2];                    /* words 5, 6 */
} iem_mpc_state_t;
int iem_mpc_create(iem_amu *a, const iem_mpc_opts_t *opts, iem_mpc **out);
int iem_mpc_destroy(iem_mpc *q);
int iem_mpc_reset(iem_mpc *q);
int iem_mpc_bind_mu(iem_mpc *q, const iem_mu *p /* NULL unbinds */);
int iem_mpc_terms(iem_mpc *q, const double *d_x, const double *d_s, const double *d_y, const double *d_zL, const double *d_zU, const double *d_vL,
                  const double *d_vU, const double *d_r, const double *d_c, const double *d_sol_aff, const double *d_ds_aff, const double *d_dzL_aff,
                  const double *d_dzU_aff, const double *d_dvL_aff, const double *d_dvU_aff, double mu, double *d_rhs2, int64_t ld);
int iem_mpc_step(iem_mpc *q, const double *d_x, const double *d_s, const double *d_y, const double *d_zL, const double *d_zU, const double *d_vL,
                 const double *d_vU, const double *d_sol_aff, const double *d_ds_aff, const double *d_dzL_aff, const double *d_dzU_aff,
                 const double *d_dvL_aff, const double *d_dvU_aff, const double *d_sol_c, double mu, double tau, double *d_ds_c, double *d_dzL_c,
                 double *d_dzU_c, double *d_dvL_c, double *d_dvU_c, double *d_alpha_c /* 2 */);
int iem_mpc_select(iem_mpc *q, const double *d_probe4 /* q_c */, const double *d_alpha_c /* 2 */, const double *d_sol_c, const double *d_ds_c,
                   const double *d_dzL_c, const double *d_dzU_c, const double *d_dvL_c, const double *d_dvU_c, double *d_sol, double *d_ds, double *d_dzL,
                   double *d_dzU, double *d_dvL, double *d_dvU, double *d_alpha /* 2 */);
int iem_mpc_device(const iem_mpc *q, double **d_block);
int iem_mpc_state(iem_mpc *q, iem_mpc_state_t *out);      /* synchronises the stream: the one read-back */
/* HIP source of the four kernels and its cache key — for offline builds (no device needed; malloc'ed) */
int iem_mpc_source(char **out_src, uint64_t *out_key);

/* ---- the starting point: least-squares multipliers and the warm start --------------------------------------------------------------------
 * What stands in front of the first iteration (csrc/iem_init_device.h), as an object created ON an iem_barrier whose bounds, flags and
 * grid it borrows: Ipopt's default initialiser of the row multipliers (DefaultIterateInitializer::least_square_mults with
 * constr_mult_init_max) behind iem_barrier_start for a COLD start, and in the place of iem_barrier_start for a WARM start the
 * projection of a given primal-dual point (Ipopt's WarmStartIterateInitializer: warm_start_bound_push, warm_start_bound_frac,
 * warm_start_mult_bound_push, warm_start_mult_init_max) with a barrier parameter taken from that point's complementarity.
 *
 * Entry order and flags (fx / fc) are those of iem_barrier_terms: one thread takes the entries i, i + stride, ... of
 * [0, nvar + ncon); nothing is read where no bound is present; entries of s, vL, vU on equality rows are neither read nor written.
 * Each operation is rounded once, in the order written here.
 *
 * THE LEAST-SQUARES ESTIMATE.  With grad f + J'y − zL + zU = 0 and −y − vL + vU = 0 on inequality rows, y_new = y + delta minimises
 *         ‖r + J'delta − zL + zU‖² + ‖−(y + delta) − vL + vU‖² (the second term over inequality rows),
 *     r = obj_weight·grad f + J'y as iem_eval_residual writes it (at y = 0: the gradient).  Its normal equations are the existing K
 *     with a ZERO Hessian value array, sigma = 1, dcon = 1 on inequality rows and 0 on equality rows, delta_w = 0:
 *         [I, J'; J, −diag(dcon + delta_c)] [w; delta] = [−(r − zL + zU); t + y (inequality rows), 0 (equality rows)],
 *         t = (lower ? vL : 0) − (upper ? vU : 0).
 * iem_init_ls_terms: ONE launch on the barrier object's grid.  variables: sigma = 1.0;  a = r − zL (lower bound present);
 *     a = a + zU (upper bound present);  rhs = −a.  equality rows: dcon = +0.0, rhs = +0.0.  inequality rows: dcon = 1.0,
 *     t = (lower ? vL : +0.0) − (upper ? vU : +0.0);  rhs = y + t.  The caller assembles with a zeroed hess array
 *     (iem_kkt_assemble_diag(k, zeros, jac, sigma, dcon, 0, delta_c)), factors and solves with the existing calls; the refined solve
 *     stays matrix-free at (x, y = 0, obj_weight = 0), where the Hessian of the Lagrangian is zero.
 * iem_init_ls_apply: an 8-byte device-to-device copy (the seed of the maximum, +0.0) and at most two launches on the same grid.  The norm:
 *     yn = y + sol[nvar + j] over ALL rows, ynorm = max |yn| as an integer maximum on the bit patterns — order-independent, a NaN
 *     wins, at most one atomic per workgroup; without rows it is +0.0 and this launch is left out.  The apply: every thread reads
 *     ynorm; ACCEPTED iff ynorm <= y_max (a NaN compares false).  Accepted: y = yn.  Rejected with on_reject = 0: y = +0.0 (Ipopt's
 *     initialiser); with on_reject = 1 the call returns before its first store to y (Ipopt's recalc_y use).  sol's x part is never
 *     read.  One thread writes words 0–3 of the own block.
 * iem_init_warm: ONE launch, in place.  x takes the projection of iem_barrier_start with (warm_push, warm_frac) in the place of
 *     (bound_push, bound_frac) — with equal constants the bits of iem_barrier_start — and s on inequality rows the same projection
 *     of THE GIVEN s (not of c).  Each present bound multiplier (zL, zU; vL, vU on inequality rows):
 *         z = (z > warm_z_push) ? z : warm_z_push   (a NaN becomes the push);   z = (z < warm_z_max) ? z : warm_z_max;
 *     each absent one becomes +0.0.  Every row's y:  y = NaN ? +0.0 : (y < −warm_y_max) ? −warm_y_max : (y > warm_y_max) ? warm_y_max : y.
 * iem_init_mu(q, w12, p): ONE workgroup of 64 threads, one thread decides.  w12: the twelve words of iem_mu_error at the warm state;
 *     nz of iem_barrier_info.  If nz == 0, or w[10] != 0, or avg = w[9]/nz is a NaN or not > 0:  mu0 = p's mu_init (word 5 = 1).
 *     Otherwise t = mu_factor·avg;  mu0 = t (word 5 = 0);  t > cap: mu0 = cap (3);  then mu0 < mu_floor: mu0 = mu_floor (2) — cap =
 *     mu_cap, or p's mu_init where mu_cap is 0; mu_floor that of p.  Words 0–2 and 8–11 of p's block are then written bit for bit as
 *     iem_mu_reset(p, mu0) writes them (mu0, max(tau_min, 1 − mu0), sqrt(mu0); status ITERATING, flags and counters 0); words 3–7
 *     stay.  The objects bound to p read the new mu with their next launch; iem_amu / iem_qf / iem_search keep their own resets.
 * THE OWN BLOCK: sixteen 8-byte words on the device (iem_init_device gives the pointer; iem_init_state_t mirrors words 0–5):
 *     0 ynorm of the last iem_init_ls_apply      1 its decision (int64): 1 accepted, 0 rejected      2 estimates accepted so far (int64)
 *     3 rejected so far (int64)      4 the mu0 last written by iem_init_mu      5 how it was chosen (int64): 0 from the average,
 *     1 fallback to mu_init, 2 clamped below, 3 clamped above      6–15 zero
 *     iem_init_create zeroes it; iem_init_reset (one launch of one workgroup of 64 threads, asynchronous) does the same.
 * iem_init_state: the one read-back (one synchronisation).
 * Every other call runs on the handle's stream, asynchronous, capturable; nothing allocates after create.  No float atomic, no
 * cooperative launch.  IEM_E_ARG before any device work: null required pointers (s, vL, vU may be NULL without inequality rows; y,
 * dcon without rows), an option that is not finite or outside its range (below), an iem_mu of another barrier object.  The object
 * borrows the iem_barrier object: destroy it first.  Not here: the delta_w / inertia retry, Ipopt's least_square_init_primal and
 * least_square_init_duals, bound_mult_init_method = mu-based, warm_start_target_mu and warm_start_entire_iterate, a warm start of
 * iem_resto, sharded handles.  iem_barrier_start is unchanged. */
typedef struct iem_init iem_init;
typedef struct {
  uint64_t struct_size;                 /* set by the CALLER to sizeof(iem_init_opts_t) */
  double y_max;                         /* 1e3 (Ipopt's constr_mult_init_max); >= 0 */
  int64_t on_reject;                    /* 0: a rejected estimate writes y = +0.0; 1: it keeps y */
  double warm_push, warm_frac;          /* 1e-3, 1e-3; > 0, in (0, 0.5] */
  double warm_z_push, warm_z_max;       /* 1e-3, 1e6; > 0, >= warm_z_push */
  double warm_y_max;                    /* 1e6; > 0 */
  double mu_factor;                     /* 1.0; > 0 */
  double mu_cap;                        /* 0 = the mu_init of the iem_mu object handed to iem_init_mu; >= 0 */
} iem_init_opts_t;                      /* NULL = the defaults */
typedef struct {
  uint64_t struct_size;                 /* set by the CALLER to sizeof(iem_init_state_t): at most that many bytes are written */
  double ynorm;                         /* word 0 */
  int64_t accepted, n_accepted, n_rejected;      /* words 1–3 */
  double mu0;                           /* word 4 */
  int64_t how;                          /* word 5 */
} iem_init_state_t;
int iem_init_create(iem_barrier *b, const iem_init_opts_t *opts, iem_init **out);
int iem_init_destroy(iem_init *q);
int iem_init_reset(iem_init *q);
int iem_init_ls_terms(iem_init *q, const double *d_y, const double *d_zL, const double *d_zU, const double *d_vL, const double *d_vU, const double *d_r,
                      double *d_sigma, double *d_dcon, double *d_rhs);
int iem_init_ls_apply(iem_init *q, const double *d_sol, double *d_y);
int iem_init_warm(iem_init *q, double *d_x, double *d_s, double *d_y, double *d_zL, double *d_zU, double *d_vL, double *d_vU);
int iem_init_mu(iem_init *q, const double *d_out12 /* of iem_mu_error */, iem_mu *p);
int iem_init_device(const iem_init *q, double **d_block);
int iem_init_state(iem_init *q, iem_init_state_t *out);      /* synchronises the stream: the one read-back */
/* HIP source of the six kernels and its cache key — for offline builds (no device needed; malloc'ed) */
int iem_init_source(char **out_src, uint64_t *out_key);

/* ---- the stopping test and the kept iterate -----------------------------------------------------------------------------------------------
 * What decides that a solve ends (csrc/iem_conv_device.h), as an object created ON an iem_mu whose barrier object, grid, tol, s_max and
 * mu_floor it borrows and whose block it reads: Ipopt's OptimalityErrorConvergenceCheck — the scaled error E(0) beside the unscaled
 * tolerances (dual_inf_tol, constr_viol_tol, compl_inf_tol), the ACCEPTABLE level (acceptable_tol and its companions, met
 * acceptable_iter times in a row), max_iter, diverging_iterates_tol, the invalid number and the tiny step — and THE KEPT ITERATE: the
 * best acceptable point, copied into the object's own buffers on the device's own decision, without a read-back, and handed back
 * when the solve later stalls, diverges, runs out of iterations or fails in restoration.  iem_mu_update keeps its own test
 * (E(0) <= tol) and its status word; this object neither reads nor writes them.
 *
 * Entry order and flags (fx / fc) are those of iem_barrier_terms: one thread takes the entries i, i + stride, ... of
 * [0, nvar + ncon); nothing is read where no bound is present; entries of s, vL, vU, ds on equality rows are neither read nor
 * written.  Each operation is rounded once, in the order written here.  The maxima are integer maxima on the bit patterns of
 * non-negative doubles — order-independent, a NaN wins, at most one atomic per workgroup and slot.
 *
 * THE BLOCK: twenty-four 8-byte words on the device (iem_conv_device gives the pointer; iem_conv_state_t mirrors words 0–18).
 *     int64:  0 status: 0 ITERATING, 1 CONVERGED, 2 ACCEPTABLE, 3 MAXITER, 4 DIVERGING, 5 INVALID, 6 TINY_STEP
 *             1 checks so far      2 acceptable checks in a row      3 keep: the last check asks for a copy      4 kept: a point is held
 *             5 the value of word 1 at the check that kept it      6 flags: bit 0 = acceptable now, bit 1 = this step tiny, bit 2 = tiny
 *             with mu above its floor (the hint for force_fixed of iem_amu_update / iem_qf_update)      7 tiny steps in a row
 *     double: 8 E(0)      9 d = max(w0, w1)      10 p = ncon ? w2 : 0      11 cpl = nz ? w3 : 0      12 f      13 the f of the previous
 *             check (what the objective change was taken against)      14 xmax      15 E(0) of the kept point      16 its f      17 rel
 *             18 dymax      19–23 zero
 *     A status other than 0 is LATCHED: every later iem_conv_check writes keep = 0 and nothing else, every later iem_conv_step writes
 *     nothing, until iem_conv_reset (one launch of one workgroup of 64 threads: the block zero; the kept buffers keep their bytes).
 * iem_conv_check(q, w12, f, x): an 8-byte device-to-device copy (the seed of the maximum, +0.0) and two launches.  xmax = max_i |x_i|
 *     over the variables.  Then one thread decides.  E(0) in the expressions of iem_mu_update at mu = +0.0 with that object's s_max:
 *     word 8 is bit for bit word 3 of the iem_mu block after iem_mu_update on the same twelve words.  The first branch that applies:
 *     1. w[10] != 0, or one of E(0), f, xmax a NaN, or E(0) or f infinite: INVALID (keep = 0, bit 0 clear).
 *     2. E(0) <= tol && d <= dual_inf_tol && p <= constr_viol_tol && cpl <= compl_inf_tol: CONVERGED, keep = 1 (bit 0 clear: the
 *        acceptable level is not evaluated, the count of word 2 stays).
 *     3. acceptable = E(0) <= acceptable_tol && d <= acceptable_dual_inf_tol && p <= acceptable_constr_viol_tol && cpl <=
 *        acceptable_compl_inf_tol && (word 1 == 0, the first check of a solve, or |f − f_prev| / max(1, |f|) <= acceptable_obj_change_tol,
 *        f_prev the f of the previous check).  Bit 0 = acceptable; word 2 grows by one when acceptable and returns to 0 when not.
 *        acceptable && (kept == 0 || E(0) <= word 15): keep = 1.  acceptable_iter > 0 && word 2 >= acceptable_iter: ACCEPTABLE.
 *     4. otherwise word 1 >= max_iter: MAXITER (max_iter iterations pass; the check behind them stops).
 *     5. otherwise xmax > diverging_iterates_tol: DIVERGING.
 *     keep is written 0 or 1 by every check; with keep = 1, kept = 1 and words 15, 16, 5 take E(0), f and word 1.  Words 8–14 are
 *     rewritten by every unlatched check; word 1 grows by one where the status stays 0.  Bits 1 and 2 of the flags stay.
 * iem_conv_keep(q, state): ONE launch on the barrier grid.  Every thread reads keep, which the launch does not write; at 0 it
 *     returns before its first store.  At 1 it copies into the object's own buffers (3 nvar + 4 ncon doubles, allocated and zeroed at
 *     create): x; zL / zU where the bound is present, +0.0 where absent; every row's y; s, vL, vU of inequality rows the same way.
 * iem_conv_restore(q, state): the same launch in the other direction on the word kept; at 0 it touches nothing; where it copies it
 *     writes only the entries that iem_conv_keep reads.  iem_conv_kept hands out the seven device pointers (any may be NULL).
 * iem_conv_step(q, x, s, sol, ds): after the direction is solved; a 16-byte seed copy and two launches.
 *     rel = max(|sol_i| / (1.0 + |x_i|) over the variables, |ds_j| / (1.0 + |s_j|) over the inequality rows);  dymax = max_j |sol[nvar + j]|
 *     over all rows.  tiny = rel < tiny_step_tol (a NaN compares false); word 7 grows when tiny, otherwise returns to 0; bit 1 = tiny;
 *     bit 2 = tiny && mu > mu_floor, mu = word 0 of the iem_mu block; word 7 >= 2 && dymax < tiny_step_y_tol && mu <= mu_floor:
 *     TINY_STEP.  Ipopt also skips its line search on a tiny step; this object only reports.
 * iem_conv_state: the one read-back (one synchronisation).
 * Every other call runs on the handle's stream, asynchronous, capturable; nothing allocates after create.  No float atomic, no
 * cooperative launch.  IEM_E_ARG before any device work: null required pointers (s, vL, vU, ds may be NULL without inequality rows, y
 * without rows), a tolerance that is <= 0 or a NaN (+inf is allowed and switches that test off), a negative max_iter or
 * acceptable_iter, a struct_size that is not the struct's.  The object borrows the iem_mu object: destroy it first.  Not here: the
 * delta_w / inertia retry, Ipopt's skipping of the line search on a tiny step, max_cpu_time, a freeze of the other kernels behind the
 * latch (a replay past a terminal status keeps iterating; iem_conv_restore is what hands back the point),
 * scaled against unscaled problems (the tolerances apply in the scaling the caller evaluates in), sharded handles. */
typedef struct iem_conv iem_conv;
typedef struct {
  uint64_t struct_size;                 /* set by the CALLER to sizeof(iem_conv_opts_t) */
  double dual_inf_tol, constr_viol_tol, compl_inf_tol;      /* 1, 1e-4, 1e-4; > 0, +inf allowed */
  double acceptable_tol;                /* 1e-6 */
  int64_t acceptable_iter;              /* 15; 0 switches the ACCEPTABLE stop off (points are still kept); >= 0 */
  double acceptable_dual_inf_tol, acceptable_constr_viol_tol, acceptable_compl_inf_tol, acceptable_obj_change_tol;      /* 1e10, 1e-2, 1e-2, 1e20 */
  int64_t max_iter;                     /* 3000; >= 0 */
  double diverging_iterates_tol;        /* 1e20 */
  double tiny_step_tol, tiny_step_y_tol;                    /* 10·2^-52, 1e-2 */
} iem_conv_opts_t;                      /* NULL = the defaults */
typedef struct {
  uint64_t struct_size;                 /* set by the CALLER to sizeof(iem_conv_state_t) */
  int64_t status, checks, acceptable_count, keep, kept, kept_at, flags, tiny_count;      /* words 0–7 */
  double e0, dual_inf, constr_viol, compl_inf, f, f_prev, xmax, kept_e0, kept_f, rel, dymax;      /* words 8–18 */
} iem_conv_state_t;
int iem_conv_create(iem_mu *p, const iem_conv_opts_t *opts, iem_conv **out);
int iem_conv_destroy(iem_conv *q);
int iem_conv_reset(iem_conv *q);
int iem_conv_check(iem_conv *q, const double *d_out12 /* of iem_mu_error */, const double *d_f /* 1 */, const double *d_x);
int iem_conv_keep(iem_conv *q, const double *d_x, const double *d_s, const double *d_y, const double *d_zL, const double *d_zU, const double *d_vL, const double *d_vU);
int iem_conv_restore(iem_conv *q, double *d_x, double *d_s, double *d_y, double *d_zL, double *d_zU, double *d_vL, double *d_vU);
int iem_conv_step(iem_conv *q, const double *d_x, const double *d_s, const double *d_sol, const double *d_ds);
int iem_conv_kept(const iem_conv *q, double **d_x, double **d_s, double **d_y, double **d_zL, double **d_zU, double **d_vL, double **d_vU);
int iem_conv_device(const iem_conv *q, double **d_block);
int iem_conv_state(iem_conv *q, iem_conv_state_t *out);      /* synchronises the stream: the one read-back */
/* HIP source of the seven kernels and its cache key — for offline builds (no device needed; malloc'ed) */
int iem_conv_source(char **out_src, uint64_t *out_key);

/* ---- the restoration phase's barrier parameter ---------------------------------------------------------------------------------------
 * The restoration problem's own mu on the device (csrc/iem_rmu_device.h), as an object created ON an iem_resto: Ipopt's monotone rule
 * for the restoration problem, the exit "converged to a point of local infeasibility" (STATIONARY), the start of a phase
 * (mu_R = max(mu, max |inf|)), Ipopt's alpha_min rule behind an iem_search_accept, and the BOUND variant of the restoration code
 * object, whose kernels read mu, tau and zeta from a block instead of host doubles.  One captured restoration iteration
 *     iem_eval_residual(0);  iem_rmu_error;  iem_rmu_update;  iem_jac_hess_coord(0);  iem_resto_terms;  assemble;  factor;  refined solve;
 *     iem_resto_step;  iem_resto_merit(0);  iem_resto_begin;  K x { iem_resto_trial, iem_cons, iem_resto_merit(1), iem_search_accept(inner),
 *     iem_rmu_trigger(1) };  iem_resto_update;  iem_obj_device;  iem_cons;  iem_barrier_merit;  iem_resto_check
 * then replays across a change of the restoration's mu, and the host reads one struct per iteration (iem_rmu_state).
 *
 * The object owns a genuine iem_mu object on the same barrier object — the RESTORATION BLOCK, the sixteen words of the iem_mu block,
 * built by iem_mu_create with the options below; iem_rmu_mu returns it (never to be destroyed by the caller; iem_mu_device,
 * iem_mu_state and iem_search_bind_mu(inner, ...) apply to it) — and its OWN BLOCK of sixteen 8-byte words (iem_rmu_device):
 *     0 status (int64): 0 ITERATING, 1 STATIONARY, 2 UNUSABLE      1 flags (int64): bit 0 = mu changed in the last update, bit 1 = the
 *     ladder of the last update was truncated      2 decreases in the last update (int64)      3 decreases since enter (int64)
 *     4 E_R(0)      5 E_R(mu) at the mu the update leaves      6 mu at enter      7 max |inf| at enter
 *     8 alpha_min of the last trigger call that evaluated it      9 triggers fired on the original search (int64)
 *     10 triggers fired on the inner search (int64)      11-15 zero
 * IEM_RMU_K = 6 candidates is a compile-time constant: one update decreases mu at most IEM_RMU_K − 1 = 5 times.
 * iem_rmu_enter(d_err: the 8 words of iem_barrier_error or the first 8 of iem_mu_error at this point; mu_host): one workgroup, one
 *     thread decides.  mu_orig = word 0 of the original block when par_orig was given, otherwise mu_host;  mu_R = max(mu_orig, d_err[2])
 *     (a NaN propagates).  mu_R a NaN or not > 0: status UNUSABLE and nothing else moves.  Otherwise the restoration block is written bit
 *     for bit as iem_mu_reset(p, mu_R) writes it, the own block is zeroed except word 6 = mu_R and word 7 = d_err[2], and words 11, 12
 *     of the inner search's control block are zeroed (the 16 bytes of iem_search_reset).  Issue it in front of iem_resto_enter: bound,
 *     that call takes mu_R from the block.  The trigger counters (words 9, 10) start from zero with the phase: a caller who counts over a
 *     whole solve reads them (iem_rmu_state) in front of the next iem_rmu_enter and carries them over.
 * iem_rmu_error: ONE launch on the barrier object's grid behind one 256-byte device-to-device copy (the seed), 32 words.  The
 *     candidates  mu_0 = word 0, zeta_0 = word 2 of the restoration block,  mu_{k+1} = max(mu_floor, min(kappa_mu·mu_k,
 *     mu_k·sqrt(mu_k))),  zeta_{k+1} = sqrt(mu_{k+1})  are formed once per thread.  With E the output of iem_resto_error:
 *     [0]-[7] bit for bit iem_resto_error(mu = 0, zeta = zeta_0) on the same inputs (same per-lane order, same fixed-order totals; the
 *     partial sums are the restoration block's own)  [8] the minimum, [9] the sum, [10] the count of unusable values of the
 *     complementarity products exactly as iem_mu_error defines its words 8-10, taken over the present bounds AND p·zp, n·zn on every
 *     row (a lane's entries in index order; per row the slack's bounds, then p·zp, then n·zn)  [11] +0.0
 *     [12 + 3k] mu_k, [13 + 3k] E[0] at zeta_k, [14 + 3k] E[1] at zeta_k for k = 0..5 (integer maxima on bit patterns: a NaN gives a NaN)
 *     [30], [31] +0.0.  d_r is required: no NaN form.
 * iem_rmu_update(d_out32): one workgroup, one thread decides, each operation rounded once, every max / min propagating a NaN.  With w
 *     the 32 words, m = ncon and nzr = nz + 2·ncon:
 *         sd = max(s_max, (w4 + w5)/max(1, m + nzr))/s_max      sc = max(s_max, w5/max(1, nzr))/s_max
 *         E_k(mu) = max(max(max(w[13+3k], w[14+3k])/sd, m ? w2 : 0), nzr ? max(w3 − mu, mu − w8)/sc : 0)
 *     w10 != 0 or E_0(0) a NaN: UNUSABLE.  Else E_0(0) <= tol: STATIONARY.  In both the restoration block and the filter stay (j = 0).
 *     Else ITERATING and  j = 0;  while j < 5 and mu_j > mu_floor and E_j(mu_j) <= kappa_eps·mu_j:  j += 1  (mu_j = w[12+3j]); when
 *     the condition still holds at j = 5, flag bit 1 is set (otherwise cleared) and the next update goes on from there.  j > 0: words
 *     0-2 of the restoration block become mu_j, max(tau_min, 1 − mu_j), sqrt(mu_j), flag bit 0 is set, word 2 = j, word 3 grows by j,
 *     and the inner filter is emptied.  j = 0: flag bit 0 is cleared, word 2 = 0, block and filter stay untouched.  Status, word 4 =
 *     E_0(0) and word 5 = E_j(mu_j) are stored either way.  The status is not latched: the next update decides again.
 * iem_rmu_trigger(which: 0 the original search of the iem_resto, 1 its inner search; d_alpha: that search's step lengths): one
 *     workgroup of 64 behind an iem_search_accept.  With a status other than SEARCHING it writes nothing.  Otherwise, with that
 *     search's options and words 0 (alpha), 3 (theta0), 4 (slope), 5 (theta_min) of its control block:  a = gamma_theta;  slope < 0:
 *     a = min(a, (gamma_phi·theta0)/(−slope));  slope < 0 and theta0 <= theta_min:  a = min(a, (delta·pow(theta0, s_theta))/pow(−slope,
 *     s_phi));  alpha_min = gamma_alpha·a  into word 8.  alpha < alpha_min (a NaN compares false): that search's status FAILED, its
 *     word 0 = +0.0, d_alpha[0] = +0.0, counter 9 + which grows.  Idempotent.  Issued behind every accept it is Ipopt's rule exactly;
 *     issued once per captured ladder of `rungs` accepts it lets at most rungs − 1 further halvings through.  No kernel of iem_search
 *     changes.
 * iem_rmu_state: the one read-back — one gather launch, ONE copy, one synchronisation: the own block, the restoration block and
 *     the block of the iem_resto.
 * iem_resto_bind_mu(q, rp; NULL unbinds): no launch; the first bind of a handle loads the bound variant of the restoration code
 *     object (iem_resto_mu_source: the ONE text of iem_resto_source with RestoArgs two pointers longer and the reads edited), so bind
 *     outside a capture.  While bound, resto_enter / _terms / _step / _begin / _update / _error read mu from word 0 of the restoration
 *     block, resto_step tau from word 1, and every kernel that takes zeta (terms, step, merit, begin, error) reads it from word 2 —
 *     once, where the kernel read its argument before; resto_check reads the ORIGINAL problem's mu from word 0 of par_orig's block when
 *     iem_rmu_create was given one and keeps its host argument otherwise.  The host's mu / tau / zeta arguments and their range checks
 *     are ignored.  Unbound, every iem_resto_* call writes the bits it wrote before; iem_resto_source and its key are unchanged.  The
 *     inner search is bound with iem_search_bind_mu(inner, the object iem_rmu_mu returns).
 * Every call but iem_rmu_state runs on the handle's stream, asynchronous, capturable; nothing allocates after create.  No float atomic,
 * no cooperative launch.  IEM_E_ARG before any device work: null required pointers, an option that is not finite, not positive, or
 * (kappa_mu, tau_min, gamma_alpha) not below 1, a par_orig or a bind across two objects, which outside {0, 1}.  The object borrows the
 * iem_resto (destroy it first); iem_rmu_destroy unbinds that iem_resto and its inner search where they still read the block.  Not
 * here: adaptive rules for the restoration, the restoration's own second-order correction, a nested restoration, the delta_w /
 * inertia retry, a warm start of iem_resto, sharded handles. */
#define IEM_RMU_K 6
typedef struct iem_rmu iem_rmu;
typedef struct {
  uint64_t struct_size;                 /* set by the CALLER to sizeof(iem_rmu_opts_t) */
  double kappa_eps, kappa_mu, tau_min, tol, mu_floor, s_max, gamma_alpha;
} iem_rmu_opts_t;                       /* NULL = 10, 0.2, 0.99, 1e-8, 1e-11, 100, 0.05 */
typedef struct {
  uint64_t struct_size;                 /* set by the CALLER to sizeof(iem_rmu_state_t): at most that many bytes are written */
  int64_t status, flags, decreases_last, decreases;        /* words 0–3 of the own block */
  double e0, e_mu, mu_enter, inf_enter, alpha_min;         /* words 4–8 */
  int64_t triggers_orig, triggers_inner;                   /* words 9, 10 */
  double mu, tau, zeta, mu_e0, mu_e_mu, mu_e_d, mu_e_p, mu_e_c0;      /* words 0–7 of the restoration block */
  int64_t mu_status, mu_flags, mu_decreases, mu_updates;   /* words 8–11 of the restoration block */
  int64_t resto_state;                  /* word 0 of the iem_resto block */
  double theta_start, theta, phi;       /* words 1–3 of the iem_resto block */
} iem_rmu_state_t;
enum { IEM_RMU_ITERATING = 0, IEM_RMU_STATIONARY = 1, IEM_RMU_UNUSABLE = 2 };
int iem_rmu_create(iem_resto *q, const iem_mu *par_orig /* may be NULL */, const iem_rmu_opts_t *opts, iem_rmu **out);
int iem_rmu_destroy(iem_rmu *rp);
int iem_rmu_mu(const iem_rmu *rp, const iem_mu **out_par);      /* the restoration block's object: owned by rp, never to be destroyed */
int iem_rmu_enter(iem_rmu *rp, const double *d_err /* 8 */, double mu_host);
int iem_rmu_error(iem_rmu *rp, const double *d_x, const double *d_s, const double *d_y, const double *d_zL, const double *d_zU, const double *d_vL,
                  const double *d_vU, const double *d_r, const double *d_c, double *d_out /* 32 */);
int iem_rmu_update(iem_rmu *rp, const double *d_out32);
int iem_rmu_trigger(iem_rmu *rp, int which, double *d_alpha /* 2 */);
int iem_rmu_device(const iem_rmu *rp, double **d_block);
int iem_rmu_state(iem_rmu *rp, iem_rmu_state_t *out);      /* synchronises the stream: the one read-back */
int iem_resto_bind_mu(iem_resto *q, const iem_rmu *rp /* NULL unbinds */);
/* HIP source of the five kernels and its cache key — for offline builds (no device needed; malloc'ed) */
int iem_rmu_source(char **out_src, uint64_t *out_key);
/* ... and of the BOUND variant of the restoration code object; iem_resto_bind_mu loads it.  iem_resto_source, its key and the unbound
 * calls are unchanged */
int iem_resto_mu_source(char **out_src, uint64_t *out_key);

/* ---- kernel generation (no device needed) ---------------------------------------
 * The evaluator of a model is specialised HIP source generated from its templates
 * and compiled for gfx950 (offline into a code-object cache, or by hiprtc on a cache
 * miss).  These two calls expose the generator so a build step can pre-compile. */
int iem_emit_source(const void *blob, size_t nbytes, char **out_src, uint64_t *out_key);
/* The hand-written code objects whose source depends on no model and no shape, as a list — what iem_kkt_diag_source,
 * iem_kkt_border_source and iem_barrier_source return one by one: index 0, 1, .. gives the object's name
 * (*out_name: a static string, not to be freed — "kkt_diag", "kkt_border", "barrier"), its HIP source (malloc'ed)
 * and its cache key.  IEM_E_ARG for an index below 0 or past the last object, with nothing written: an offline build loops until
 * then and needs no edit when the library gains an object.  Any output pointer may be NULL. */
int iem_fixed_source(int index, const char **out_name, char **out_src, uint64_t *out_key);
/* text description of the launches (kernel name, grid, argument tables) — for tooling/tests */
int iem_emit_launch_plan(const void *blob, size_t nbytes, char **out_txt);
/* Hessian structure of a blob under the current options, computed on the host (tooling/tests;
 * arrays are malloc'ed, release with iem_free). */
int iem_blob_hess_structure(const void *blob, size_t nbytes, int base, int64_t **out_rows, int64_t **out_cols, int64_t *out_nnz);
/* structure of one explicit θ block (iem_jacp_structure / iem_hessxp_structure / iem_hesspp_structure) from a blob alone, no
 * device: which = 0 dc/dθ, 1 d2L/dx dθ, 2 d2L/dθ2.  The arrays are released with iem_free. */
int iem_blob_param_coord_structure(const void *blob, size_t nbytes, int which, int base, int64_t **out_rows, int64_t **out_cols, int64_t *out_nnz);
/* values of model array `id` as the library sees it after parsing — including the float columns it
 * synthesises when it recovers a product lattice from a flat iterator (tooling/tests; malloc'ed) */
int iem_blob_array(const void *blob, size_t nbytes, int id, double **out_vals, int64_t *out_n);
void iem_free(void *p);

/* knobs: iem_set_option changes the PROCESS DEFAULTS that iem_create and iem_emit_* read; per-handle
 * values go through iem_create_opts (defaults in csrc/iem_codegen.hpp):
 *   "store_mode"   0 direct strided stores, 1 wave-level LDS-transposed stores, 2 (default)
 *                  workgroup-staged stores re-cut at 128-byte lines
 *   "overlap"      1 (default): block-store kernels overlap their tiles by 16 lanes so that every
 *                  128-byte line is written whole by one workgroup
 *   "nt_stores", "lds_slots", "reorder", "min_waves"
 *   "block"        workgroup size; 0 (default) = per model: 512, or 256 when that wastes > 2 % fewer
 *                  lanes on the rows of a 2-D / 3-D support grid (5 000 x 100: 11 tiles of 496 vs 21 of 240)
 *   "fp_contract"  0 (default): no FMA contraction — bit-comparable with the CPU oracle
 *   "split_small"  support grids of at most this many workgroups (default 64) run their templates
 *                  side by side in one launch instead of fused lane-wise (0: never)
 *   "fuse_groups"  1 (default): one launch per call even across several support grids
 *   "fuse_zero"    1 (default): scatter kernels zero untouched output entries themselves
 *   "poll_obj"     1 (default): iem_obj polls the mapped host scalar instead of a stream sync
 *   "xcd_remap", "wide_stores" (16-byte block stores): 0 (default), measured no gain;
 *   "no_fuse", "ablate": experiments / baselines only
 *   "hess_merge"   1 selects the opt-in MERGED Hessian layout (duplicate (row,col) slots of one
 *                  support summed in registers: fewer nnzh, not ExaModels' COO layout —
 *                  hess_structure!/hess_coord! stay mutually consistent).
 *   "obj_wgs"      at most this many workgroups walk the objective's tiles (default 1024; fixed, so the
 *                  summation order is — obj is bitwise reproducible)
 *   "det_shared"   1 (default): gradient / J'v / Hv entries shared by many items are reduced in a fixed
 *                  order (no float atomics); 0: one f64 atomic per wave (A/B runs)
 *   "pull_scatter" 1 (default): grad!/jtprod!/hprod! compute a stencil neighbour's addend (x[i-1] of a difference
 *                  row) on the neighbour's lane — exclusive stores, no zero fill; 0: atomics (A/B runs)
 *   "fold_colloc"  orthogonal-collocation models: the node x element boxes of the derivative rows ride on the lanes of the
 *                  support grid.  1: for grad!/jtprod!/hprod! (with the element lists of constant_over_collocation) — every
 *                  addend on the lane that owns its entry, exclusive stores, no gather plan; 2 (default): also for every
 *                  other kind (shared loads); 0: off.  "fold_max_n" (6): at most this many rows per element
 *   "det_scatter"  1 (default): scatter addends that would still be float atomics AND can meet more than one other addend in
 *                  their entry (collocation stencils, gathered indices) are parked per item and summed per entry in the
 *                  order of a plan built at create time (12 bytes of plan + 8 of scratch per addend, at most
 *                  "det_scatter_max" = 2^28 addends per kind); 2: every remaining atomic; 0: f64 atomics
 *   "det_axis"     1 (default): grad!/jtprod!/hprod! sums over a non-lane axis (an entry that depends on t only, summed over
 *                  scenarios) are parked per item and reduced in row order by a follow-up kernel; 0: f64 atomics
 *   "lazy_loads"   2 (default): product / scatter kernels with >= "lazy_min_loads" (48) loads emit a load where its value
 *                  is first used instead of at the head of the kernel (register pressure); 1: only rows of v / y; 0: never
 *   "big_batch_jac", "big_batch_hess", "big_tile", "big_batch_slots", "big_xcd"   the LARGE-GRID shape of jac_coord! /
 *                  hess_coord!: when a kind has a support grid of at least this many workgroups (defaults 4000 / 4000 — about
 *                  2e6 quadrotor supports, outputs far beyond the Infinity Cache; 0: never), all kernels of that kind run
 *                  "big_tile"-lane workgroups (1024; 0 = the model's own; the other kinds keep theirs), stage
 *                  "big_batch_slots" (48) values per barrier pair — one 96-KB workgroup per CU — and ("big_xcd" = 1) walk their
 *                  tiles XCD-aware.  A function of kind and grid sizes only, never of a timer
 *   "pair_kernel"  1 (default): the handle also carries the fused jac + hess launch behind iem_jac_hess_coord
 *   "comm_timeout_ms"  bound of every mailbox wait of this handle's exchange kernels (default 5000)
 *   "autotune"     0 (default) / 1 (opt-in): handles whose jac/hess grid has >= "autotune_min_blocks" (400) workgroups
 *                  keep a second code object with a 48-slot LDS store batch and choose per output buffer,
 *                  from the first twenty calls into it (HIP events, every call a valid evaluation), which of
 *                  the two writes that buffer faster (the buffer's physical placement decides,
 *                  by up to 10 %).  Both variants write identical bytes.  0: default code object only. */
int iem_set_option(const char *name, int64_t value);

/* per-kernel timing of the last jac/hess call pair, measured with HIP events on the
 * handle's stream (used by bench.py for the roofline line) */
int iem_time_kernels(iem_model *m, const double *d_x, const double *d_y, double *d_jac, double *d_hess,
                     int iters, double *h_ms_jac, double *h_ms_hess);

/* Store-batch tuner (options "autotune", "autotune_min_blocks"): which variant jac_coord! (kind 0) /
 * hess_coord! (kind 1) uses for output buffer d_vals — -1 still measuring (or tuner off / buffer not seen),
 * 0 the default code object, 1 the large-batch one.  Introspection only; results never depend on it. */
int iem_tuner_choice(iem_model *m, int kind, const double *d_vals, int *out_choice);
/* Decide NOW for these output buffers (either may be NULL): per kind, twelve launches of each of the handle's two
 * code objects — complete evaluations of jac_coord!(x) into d_jac / hess_coord!(x, y; obj_weight) into d_hess, ten of
 * them timed between one pair of events — then a stream synchronise; the next call uses the faster object.  A host
 * calls it once after allocating its COO value buffers (solver set-up); without it the first twenty calls of the solve
 * into a buffer measure.  No-op (IEM_OK) on handles without a second code object. */
int iem_tune(iem_model *m, const double *d_x, const double *d_y, double obj_weight, double *d_jac, double *d_hess);

const char *iem_last_error(void);
const char *iem_version(void);

#ifdef __cplusplus
}
#endif
#endif /* IEM_H */
