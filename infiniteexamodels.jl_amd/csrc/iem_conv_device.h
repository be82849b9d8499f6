// iem_conv_device.h — the kernels of the iem_conv object (include/iem.h): THE STOPPING TEST of a primal-dual interior-point solve on an
// iem_mu object — Ipopt's scaled error at mu = 0 beside the unscaled tolerances, the acceptable level met acceptable_iter times in a
// row, the stops max_iter, diverging iterates, invalid number and tiny step (conv_xmax / conv_decide, conv_stepmax /
// conv_step_decide), and THE KEPT ITERATE: the best acceptable point copied into the object's own buffers on the device's own
// decision (conv_keep) and handed back (conv_restore).  A code object of its own (no other source key knows of it), compiled with
// -ffp-contract=off behind the helpers of iem_device.h (everything in front of its own kernels, with IEM_TILE = 256): every line
// below is the order of operations of the contract in include/iem.h, each operation rounded once.
//
// NO FLOAT ATOMIC, no inline assembly and no scratch in this file.  The only atomic is the integer atomicMax of conv_extremes on the
// bit pattern of a non-negative double (a NaN wins) — the scheme of init_ls_norm (csrc/iem_init_device.h): the waves' values meet in
// LDS first, at most ONE per workgroup and slot, and none where a relaxed agent-scope look at the slot shows that it would not change
// it.  There is no sum.
//
// The grid of the barrier object: one thread takes the entries i, i + stride, ... of [0, nvar + ncon): i < nvar is variable i,
// otherwise row j = i − nvar; fx[i] bit 0 = lower bound present, bit 1 = upper; fc[j] the same for an inequality row's slack, bit 2 =
// equality row.  Nothing is read where no bound is present; equality rows of s, vL, vU (and ds) are neither read nor written.
// conv_decide, conv_step_decide, conv_reset: ONE workgroup of 64 threads, one thread decides — it reads the block, the slots and the
// inputs first and no word that another thread of the launch writes.

// the block: words of 8 bytes
enum { CW_STATUS, CW_CHECKS, CW_ACC_COUNT, CW_KEEP, CW_KEPT, CW_KEPT_AT, CW_FLAGS, CW_TINY_COUNT,
       CW_E0, CW_D, CW_P, CW_CPL, CW_F, CW_F_PREV, CW_XMAX, CW_KEPT_E0, CW_KEPT_F, CW_REL, CW_DYMAX, CW_WORDS = 24 };
// behind the block: the slots of the maxima (the words of the iem_conv allocation 24–26), then their seed source (+0.0 twice)
enum { CS_XMAX, CS_REL, CS_DYMAX };
#define CONV_ITERATING 0ll
#define CONV_CONVERGED 1ll
#define CONV_ACCEPTABLE 2ll
#define CONV_MAXITER 3ll
#define CONV_DIVERGING 4ll
#define CONV_INVALID 5ll
#define CONV_TINY_STEP 6ll
#define CONV_INF_BITS 0x7ff0000000000000ull

struct ConvArgs {
  const unsigned char *fx, *fc;                   // the barrier object's flags
  double *x, *s, *y, *zL, *zU, *vL, *vU;          // the caller's state (xmax, stepmax and keep read it, restore writes it)
  double *kx, *ks, *ky, *kzL, *kzU, *kvL, *kvU;   // the object's own buffers: the kept point
  const double *sol, *ds;                         // stepmax: [dx; dy] and the slack direction
  const double *w, *f;                            // decide: the twelve words of mu_error, the objective
  const double *mblk;                             // step_decide: the iem_mu block (word 0 = mu)
  double *blk;                                    // the object's own block
  unsigned long long *slot;                       // the bits of xmax, rel, dymax
  double tol, s_max, mu_floor;                    // of the iem_mu object
  double dual_inf_tol, constr_viol_tol, compl_inf_tol;
  double acceptable_tol, acceptable_dual_inf_tol, acceptable_constr_viol_tol, acceptable_compl_inf_tol, acceptable_obj_change_tol;
  double diverging_iterates_tol, tiny_step_tol, tiny_step_y_tol;
  long long acceptable_iter, max_iter;
  long long ncon, nz;
  long long nvar, n;
};

// np.maximum: a NaN in either operand gives a NaN
__device__ __forceinline__ double conv_max(double a, double b) { return (a > b || a != a) ? a : b; }
__device__ __forceinline__ double conv_abs(double a) { return __longlong_as_double(__double_as_longlong(a) & 0x7fffffffffffffffll); }
__device__ __forceinline__ unsigned long long conv_abs_bits(double a) { return (unsigned long long)__double_as_longlong(a) & 0x7fffffffffffffffull; }
__device__ __forceinline__ unsigned long long conv_umax(unsigned long long a, unsigned long long b) { return a > b ? a : b; }
__device__ __forceinline__ long long conv_word(const double *blk, int w) { return __double_as_longlong(blk[w]); }
__device__ __forceinline__ void conv_set_word(double *blk, int w, long long v) { blk[w] = __longlong_as_double(v); }
__device__ __forceinline__ bool conv_is_nan(double a) { return a != a; }
__device__ __forceinline__ bool conv_is_inf(double a) { return conv_abs_bits(a) == CONV_INF_BITS; }

// The maxima of the workgroup into their slots, which were seeded with +0.0 in front of the launch: per wave by shuffles, across the
// waves through LDS (NV·4 words), then thread s < NV holds value s of the workgroup and issues ONE integer atomic — and none where a
// relaxed agent-scope look at the slot shows that it would not change it (the slot only ever rises, so a stale look can only cost an
// atomic, never lose a value)
template <int NV>
__device__ __forceinline__ void conv_extremes(unsigned long long (&v)[NV], unsigned long long *slots, unsigned long long *lds) {
  constexpr int NW = IEM_TILE / IEM_WAVE;
#pragma unroll
  for (int s = 0; s < NV; ++s) {
    for (int o = 32; o > 0; o >>= 1) v[s] = conv_umax(v[s], __shfl_xor(v[s], o, 64));
    if (iem_lane() == 0) lds[iem_wave() * NV + s] = v[s];
  }
  __syncthreads();
  if (threadIdx.x < NV) {
    const int s = (int)threadIdx.x;
    unsigned long long b = lds[s];
    for (int w = 1; w < NW; ++w) b = conv_umax(b, lds[w * NV + s]);
    const unsigned long long cur = __hip_atomic_load(slots + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (b > cur) atomicMax(slots + s, b);
  }
}

// max_i |x_i| over the variables into its slot
extern "C" __global__ __launch_bounds__(256) void conv_xmax(const ConvArgs A) {
  __shared__ unsigned long long lds[IEM_TILE / IEM_WAVE];
  const long long stride = (long long)gridDim.x * 256;
  unsigned long long m[1] = {0ull};
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < A.n; i += stride) {
    if (i >= A.nvar) continue;
    m[0] = conv_umax(m[0], conv_abs_bits(A.x[i]));
  }
  conv_extremes<1>(m, A.slot + CS_XMAX, lds);
}

// rel = max(|sol_i| / (1 + |x_i|)) over the variables and max(|ds_j| / (1 + |s_j|)) over the inequality rows; dymax = max_j |sol[nvar + j]|
// over all rows: two slots side by side
extern "C" __global__ __launch_bounds__(256) void conv_stepmax(const ConvArgs A) {
  __shared__ unsigned long long lds[2 * (IEM_TILE / IEM_WAVE)];
  const long long stride = (long long)gridDim.x * 256;
  unsigned long long m[2] = {0ull, 0ull};
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < A.n; i += stride) {
    if (i < A.nvar) {
      const double den = 1.0 + conv_abs(A.x[i]);
      const double q = conv_abs(A.sol[i]) / den;
      m[0] = conv_umax(m[0], conv_abs_bits(q));
    } else {
      const long long j = i - A.nvar;
      m[1] = conv_umax(m[1], conv_abs_bits(A.sol[i]));
      if (A.fc[j] & 4) continue;
      const double den = 1.0 + conv_abs(A.s[j]);
      const double q = conv_abs(A.ds[j]) / den;
      m[0] = conv_umax(m[0], conv_abs_bits(q));
    }
  }
  conv_extremes<2>(m, A.slot + CS_REL, lds);
}

// THE STOPPING TEST.  E(0) in the expressions of mu_update (csrc/iem_mu_device.h) at mu = +0.0, expression for expression: word 8 is
// bit for bit word 3 of the iem_mu block after mu_update on the same twelve words.
extern "C" __global__ __launch_bounds__(64) void conv_decide(const ConvArgs A) {
  if (threadIdx.x != 0) return;
  double *blk = A.blk;
  if (conv_word(blk, CW_STATUS) != CONV_ITERATING) {      // LATCHED: keep = 0 and nothing else
    conv_set_word(blk, CW_KEEP, 0);
    return;
  }
  const double *w = A.w;
  const double s_max = A.s_max;
  const long long m = A.ncon, nz = A.nz, mnz = m + nz;
  const double sd = conv_max(s_max, (w[4] + w[5]) / (double)(mnz > 1 ? mnz : 1)) / s_max;
  const double sc = conv_max(s_max, w[5] / (double)(nz > 1 ? nz : 1)) / s_max;
  const double e_d = conv_max(w[0], w[1]) / sd;
  const double e_p = m ? w[2] : 0.0;
  const double mu = 0.0;
  const double ec0 = nz != 0 ? conv_max(w[3] - mu, mu - w[8]) / sc : 0.0;
  const double e0 = conv_max(conv_max(e_d, e_p), ec0);
  const double d = conv_max(w[0], w[1]);
  const double p = m ? w[2] : 0.0;
  const double cpl = nz != 0 ? w[3] : 0.0;
  const double f = A.f[0];
  const double xmax = __longlong_as_double((long long)A.slot[CS_XMAX]);
  const long long checks = conv_word(blk, CW_CHECKS);
  const double f_prev = blk[CW_F];      // the f of the previous check (word 12 until this check rewrites it)
  long long count = conv_word(blk, CW_ACC_COUNT), kept = conv_word(blk, CW_KEPT), kept_at = conv_word(blk, CW_KEPT_AT);
  double kept_e0 = blk[CW_KEPT_E0], kept_f = blk[CW_KEPT_F];
  long long status = CONV_ITERATING, keep = 0, acceptable = 0;
  if (w[10] != 0.0 || conv_is_nan(e0) || conv_is_nan(f) || conv_is_nan(xmax) || conv_is_inf(e0) || conv_is_inf(f)) {
    status = CONV_INVALID;
  } else if (e0 <= A.tol && d <= A.dual_inf_tol && p <= A.constr_viol_tol && cpl <= A.compl_inf_tol) {
    status = CONV_CONVERGED;
    keep = 1;
  } else {
    bool small_change = checks == 0;      // the first check of a solve has no previous objective
    if (!small_change) {
      const double diff = conv_abs(f - f_prev);
      const double den = conv_max(1.0, conv_abs(f));
      small_change = diff / den <= A.acceptable_obj_change_tol;
    }
    const bool acc = e0 <= A.acceptable_tol && d <= A.acceptable_dual_inf_tol && p <= A.acceptable_constr_viol_tol && cpl <= A.acceptable_compl_inf_tol && small_change;
    acceptable = acc ? 1 : 0;
    count = acc ? count + 1 : 0;
    if (acc && (kept == 0 || e0 <= kept_e0)) keep = 1;
    if (A.acceptable_iter > 0 && count >= A.acceptable_iter) status = CONV_ACCEPTABLE;
    else if (checks >= A.max_iter) status = CONV_MAXITER;
    else if (xmax > A.diverging_iterates_tol) status = CONV_DIVERGING;
  }
  if (keep) { kept = 1; kept_at = checks; kept_e0 = e0; kept_f = f; }
  conv_set_word(blk, CW_STATUS, status);
  conv_set_word(blk, CW_CHECKS, status == CONV_ITERATING ? checks + 1 : checks);
  conv_set_word(blk, CW_ACC_COUNT, count);
  conv_set_word(blk, CW_KEEP, keep);
  conv_set_word(blk, CW_KEPT, kept);
  conv_set_word(blk, CW_KEPT_AT, kept_at);
  conv_set_word(blk, CW_FLAGS, (conv_word(blk, CW_FLAGS) & ~1ll) | acceptable);
  blk[CW_E0] = e0;
  blk[CW_D] = d;
  blk[CW_P] = p;
  blk[CW_CPL] = cpl;
  blk[CW_F] = f;
  blk[CW_F_PREV] = f_prev;
  blk[CW_XMAX] = xmax;
  blk[CW_KEPT_E0] = kept_e0;
  blk[CW_KEPT_F] = kept_f;
}

// THE TINY STEP, after the direction is solved.  Latched: nothing is written.
extern "C" __global__ __launch_bounds__(64) void conv_step_decide(const ConvArgs A) {
  if (threadIdx.x != 0) return;
  double *blk = A.blk;
  if (conv_word(blk, CW_STATUS) != CONV_ITERATING) return;
  const double rel = __longlong_as_double((long long)A.slot[CS_REL]);
  const double dymax = __longlong_as_double((long long)A.slot[CS_DYMAX]);
  const double mu = A.mblk[0];
  const bool tiny = rel < A.tiny_step_tol;      // a NaN compares false
  const long long count = tiny ? conv_word(blk, CW_TINY_COUNT) + 1 : 0;
  const bool at_floor = mu <= A.mu_floor;
  long long flags = conv_word(blk, CW_FLAGS) & 1ll;
  if (tiny) flags |= 2ll;
  if (tiny && mu > A.mu_floor) flags |= 4ll;
  if (count >= 2 && dymax < A.tiny_step_y_tol && at_floor) conv_set_word(blk, CW_STATUS, CONV_TINY_STEP);
  conv_set_word(blk, CW_FLAGS, flags);
  conv_set_word(blk, CW_TINY_COUNT, count);
  blk[CW_REL] = rel;
  blk[CW_DYMAX] = dymax;
}

// the copy of the state into the kept buffers (RESTORE = false: on the word keep) and back (RESTORE = true: on the word kept).  Every
// thread reads the word, which the launch does not write; at 0 it returns before its first store.  keep writes +0.0 where a bound is
// absent (nothing is read there); restore writes only the entries that keep reads.
template <bool RESTORE>
__device__ __forceinline__ void conv_copy(const ConvArgs &A) {
  if (conv_word(A.blk, RESTORE ? CW_KEPT : CW_KEEP) == 0) return;
  const long long stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < A.n; i += stride) {
    if (i < A.nvar) {
      const unsigned f = A.fx[i];
      if (RESTORE) {
        A.x[i] = A.kx[i];
        if (f & 1) A.zL[i] = A.kzL[i];
        if (f & 2) A.zU[i] = A.kzU[i];
      } else {
        A.kx[i] = A.x[i];
        A.kzL[i] = (f & 1) ? A.zL[i] : 0.0;
        A.kzU[i] = (f & 2) ? A.zU[i] : 0.0;
      }
    } else {
      const long long j = i - A.nvar;
      const unsigned f = A.fc[j];
      if (RESTORE) A.y[j] = A.ky[j];
      else A.ky[j] = A.y[j];
      if (f & 4) continue;
      if (RESTORE) {
        A.s[j] = A.ks[j];
        if (f & 1) A.vL[j] = A.kvL[j];
        if (f & 2) A.vU[j] = A.kvU[j];
      } else {
        A.ks[j] = A.s[j];
        A.kvL[j] = (f & 1) ? A.vL[j] : 0.0;
        A.kvU[j] = (f & 2) ? A.vU[j] : 0.0;
      }
    }
  }
}
extern "C" __global__ __launch_bounds__(256) void conv_keep(const ConvArgs A) { conv_copy<false>(A); }
extern "C" __global__ __launch_bounds__(256) void conv_restore(const ConvArgs A) { conv_copy<true>(A); }

// a new solve: the block zero (the kept buffers keep their bytes)
extern "C" __global__ __launch_bounds__(64) void conv_reset(const ConvArgs A) {
  if (threadIdx.x < CW_WORDS) A.blk[threadIdx.x] = 0.0;
}
