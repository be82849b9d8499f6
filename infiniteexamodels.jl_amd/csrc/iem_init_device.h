// iem_init_device.h — the kernels of the iem_init object (include/iem.h): THE STARTING POINT of a primal-dual interior-point solve on
// the bounds of an iem_barrier object — the right-hand side and the diagonals of the least-squares estimate of the row multipliers
// (init_ls_terms: Ipopt's default initialiser, the existing K with a zero Hessian, sigma = 1 and dcon = 1 on inequality rows), the
// estimate's size and the decision to take it (init_ls_norm, init_ls_apply: constr_mult_init_max), the projection of a WARM start —
// the primal push of barrier_start on the given x AND the given s, the bound multipliers clamped, the row multipliers clipped
// (init_warm) — and the barrier parameter of a warm start from the complementarity average, written into the block of an iem_mu
// object bit for bit as mu_reset writes it (init_mu).  A code object of its own (no other source key knows of it), compiled with
// -ffp-contract=off behind the helpers of iem_device.h (everything in front of its own kernels, with IEM_TILE = 256): every line
// below is the order of operations of the contract in include/iem.h, each operation rounded once.
//
// NO FLOAT ATOMIC, no inline assembly and no scratch in this file.  The only atomic is the integer atomicMax of init_ls_norm on the
// bit pattern of a non-negative double (a NaN wins) — the scheme of barrier_step (csrc/iem_barrier_device.h): the waves' values
// meet in LDS first, at most ONE per workgroup, and none where a relaxed look at the slot shows that it would not change it.  There
// is no sum.
//
// The grid of the barrier object: one thread takes the entries i, i + stride, ... of [0, nvar + ncon): i < nvar is variable i,
// otherwise row j = i − nvar; fx[i] bit 0 = lower bound present, bit 1 = upper; fc[j] the same for an inequality row's slack, bit 2 =
// equality row.  Nothing is read where no bound is present; equality rows of s, vL, vU are neither read nor written.  init_mu,
// init_reset: ONE workgroup of 64 threads, one thread decides.

// the object's own block: words of 8 bytes
enum { IW_YNORM, IW_ACCEPTED, IW_N_ACCEPTED, IW_N_REJECTED, IW_MU0, IW_HOW };
// how mu0 was chosen (word 5)
#define INIT_FROM_AVERAGE 0ll
#define INIT_FALLBACK 1ll
#define INIT_CLAMPED_BELOW 2ll
#define INIT_CLAMPED_ABOVE 3ll
// the words of the iem_mu block that mu_reset writes (MW_* of csrc/iem_mu_device.h)
enum { INIT_MW_MU = 0, INIT_MW_TAU = 1, INIT_MW_ZETA = 2, INIT_MW_STATUS = 8, INIT_MW_FLAGS = 9, INIT_MW_DECREASES = 10, INIT_MW_UPDATES = 11 };

struct InitArgs {
  const double *xl, *xu, *rl, *ru, *ceq;          // the barrier object's relaxed bounds and the equality rows' right-hand side
  const unsigned char *fx, *fc;
  double *x, *s, *y, *zL, *zU, *vL, *vU;          // the state (ls_terms reads it, ls_apply writes y, warm writes all of it)
  const double *r;                                // ls_terms: obj_weight grad f + J'y (nvar)
  const double *sol;                              // ls_norm, ls_apply: [w; delta], the x part never read
  double *sigma, *dcon, *rhs;                     // ls_terms
  unsigned long long *slot;                       // the bits of ynorm (ls_norm raises it, ls_apply reads it)
  const double *w;                                // init_mu: the twelve words of mu_error
  double *mblk;                                   // init_mu: the iem_mu block
  double *blk;                                    // the object's own block
  double y_max, push, frac, z_push, z_max, y_clip, mu_factor, cap;
  double mu_init, mu_floor, tau_min;              // init_mu: of the iem_mu object
  long long on_reject, nz;
  long long nvar, n;
};

// np.maximum / np.minimum: a NaN in either operand gives a NaN
__device__ __forceinline__ double init_max(double a, double b) { return (a > b || a != a) ? a : b; }
__device__ __forceinline__ double init_min(double a, double b) { return (a < b || a != a) ? a : b; }
__device__ __forceinline__ double init_abs(double a) { return __longlong_as_double(__double_as_longlong(a) & 0x7fffffffffffffffll); }
__device__ __forceinline__ unsigned long long init_abs_bits(double a) { return (unsigned long long)__double_as_longlong(a) & 0x7fffffffffffffffull; }
__device__ __forceinline__ unsigned long long init_umax(unsigned long long a, unsigned long long b) { return a > b ? a : b; }
__device__ __forceinline__ void init_set_word(double *blk, int w, long long v) { blk[w] = __longlong_as_double(v); }

// Ipopt's projection into the interior (bar_push of csrc/iem_barrier_device.h, expression for expression: with equal constants the
// bits of barrier_start)
__device__ __forceinline__ double init_push(double v, double lo, double hi, bool has_lo, bool has_hi, double k1, double k2) {
  const bool both = has_lo && has_hi;
  if (has_lo) {
    double pl = k1 * init_max(init_abs(lo), 1.0);
    if (both) pl = init_min(pl, k2 * (hi - lo));
    v = init_max(v, lo + pl);
  }
  if (has_hi) {
    double pu = k1 * init_max(init_abs(hi), 1.0);
    if (both) pu = init_min(pu, k2 * (hi - lo));
    v = init_min(v, hi - pu);
  }
  return v;
}

// a bound multiplier of a warm start: at least the push (a NaN becomes the push), at most the cap
__device__ __forceinline__ double init_clamp(double z, double lo, double hi) {
  z = (z > lo) ? z : lo;
  return (z < hi) ? z : hi;
}

extern "C" __global__ __launch_bounds__(256) void init_ls_terms(const InitArgs A) {
  const long long stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < A.n; i += stride) {
    if (i < A.nvar) {
      const unsigned f = A.fx[i];
      A.sigma[i] = 1.0;
      double a = A.r[i];
      if (f & 1) a = a - A.zL[i];
      if (f & 2) a = a + A.zU[i];
      A.rhs[i] = -a;
    } else {
      const long long j = i - A.nvar;
      const unsigned f = A.fc[j];
      if (f & 4) {
        A.dcon[j] = 0.0;
        A.rhs[i] = 0.0;
        continue;
      }
      const double tl = (f & 1) ? A.vL[j] : 0.0, tu = (f & 2) ? A.vU[j] : 0.0;
      const double t = tl - tu;
      A.dcon[j] = 1.0;
      A.rhs[i] = A.y[j] + t;
    }
  }
}

// max_j |y_j + sol[nvar + j]| into the slot, which was zeroed in front of the launch: per wave by shuffles, across the waves through
// LDS, then ONE integer atomic per workgroup — and none where a relaxed agent-scope look at the slot shows that it would not change it
extern "C" __global__ __launch_bounds__(256) void init_ls_norm(const InitArgs A) {
  __shared__ unsigned long long lds[IEM_TILE / IEM_WAVE];
  constexpr int NW = IEM_TILE / IEM_WAVE;
  const long long stride = (long long)gridDim.x * 256;
  unsigned long long m = 0ull;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < A.n; i += stride) {
    if (i < A.nvar) continue;
    const double yn = A.y[i - A.nvar] + A.sol[i];
    m = init_umax(m, init_abs_bits(yn));
  }
  for (int o = 32; o > 0; o >>= 1) m = init_umax(m, __shfl_xor(m, o, 64));
  if (iem_lane() == 0) lds[iem_wave()] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long b = lds[0];
    for (int w = 1; w < NW; ++w) b = init_umax(b, lds[w]);
    const unsigned long long cur = __hip_atomic_load(A.slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (b > cur) atomicMax(A.slot, b);
  }
}

// Every thread reads the slot — which this launch does not write — and decides the same way; one thread of workgroup 0 writes words
// 0–3 of the object's own block (which no other thread reads).  Rejected with on_reject = 1, the call returns before its first store to y.
extern "C" __global__ __launch_bounds__(256) void init_ls_apply(const InitArgs A) {
  const double ynorm = __longlong_as_double((long long)A.slot[0]);
  const bool accepted = ynorm <= A.y_max;      // a NaN compares false
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    double *blk = A.blk;
    const long long n_acc = __double_as_longlong(blk[IW_N_ACCEPTED]) + (accepted ? 1 : 0);
    const long long n_rej = __double_as_longlong(blk[IW_N_REJECTED]) + (accepted ? 0 : 1);
    blk[IW_YNORM] = ynorm;
    init_set_word(blk, IW_ACCEPTED, accepted ? 1ll : 0ll);
    init_set_word(blk, IW_N_ACCEPTED, n_acc);
    init_set_word(blk, IW_N_REJECTED, n_rej);
  }
  if (!accepted && A.on_reject) return;
  const long long stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < A.n; i += stride) {
    if (i < A.nvar) continue;
    const long long j = i - A.nvar;
    if (accepted) A.y[j] = A.y[j] + A.sol[i];
    else A.y[j] = 0.0;
  }
}

extern "C" __global__ __launch_bounds__(256) void init_warm(const InitArgs A) {
  const long long stride = (long long)gridDim.x * 256;
  const double ny = -A.y_clip;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < A.n; i += stride) {
    if (i < A.nvar) {
      const bool hl = A.fx[i] & 1, hu = A.fx[i] & 2;
      if (hl || hu) A.x[i] = init_push(A.x[i], A.xl[i], A.xu[i], hl, hu, A.push, A.frac);
      A.zL[i] = hl ? init_clamp(A.zL[i], A.z_push, A.z_max) : 0.0;
      A.zU[i] = hu ? init_clamp(A.zU[i], A.z_push, A.z_max) : 0.0;
    } else {
      const long long j = i - A.nvar;
      const unsigned f = A.fc[j];
      const double y = A.y[j];
      A.y[j] = (y != y) ? 0.0 : ((y < ny) ? ny : ((y > A.y_clip) ? A.y_clip : y));
      if (f & 4) continue;
      const bool gl = f & 1, gu = f & 2;
      A.s[j] = init_push(A.s[j], A.rl[j], A.ru[j], gl, gu, A.push, A.frac);
      A.vL[j] = gl ? init_clamp(A.vL[j], A.z_push, A.z_max) : 0.0;
      A.vU[j] = gu ? init_clamp(A.vU[j], A.z_push, A.z_max) : 0.0;
    }
  }
}

// the barrier parameter of a warm start: mu0 from the average complementarity product, then words 0–2 and 8–11 of the iem_mu block
// as mu_reset (csrc/iem_mu_device.h) writes them at that mu0; words 3–7 stay
extern "C" __global__ __launch_bounds__(64) void init_mu(const InitArgs A) {
  if (threadIdx.x != 0) return;
  const double *w = A.w;
  double mu0 = A.mu_init;
  long long how = INIT_FALLBACK;
  if (A.nz != 0 && !(w[10] != 0.0)) {
    const double avg = w[9] / (double)A.nz;
    if (avg > 0.0) {      // a NaN compares false
      const double t = A.mu_factor * avg;
      mu0 = t;
      how = INIT_FROM_AVERAGE;
      if (t > A.cap) { mu0 = A.cap; how = INIT_CLAMPED_ABOVE; }
      if (mu0 < A.mu_floor) { mu0 = A.mu_floor; how = INIT_CLAMPED_BELOW; }
    }
  }
  double *blk = A.mblk;
  blk[INIT_MW_MU] = mu0;
  blk[INIT_MW_TAU] = init_max(A.tau_min, 1.0 - mu0);
  blk[INIT_MW_ZETA] = sqrt(mu0);
  init_set_word(blk, INIT_MW_STATUS, 0);
  init_set_word(blk, INIT_MW_FLAGS, 0);
  init_set_word(blk, INIT_MW_DECREASES, 0);
  init_set_word(blk, INIT_MW_UPDATES, 0);
  A.blk[IW_MU0] = mu0;
  init_set_word(A.blk, IW_HOW, how);
}

// a new solve: the block zero
extern "C" __global__ __launch_bounds__(64) void init_reset(const InitArgs A) {
  if (threadIdx.x < 16) A.blk[threadIdx.x] = 0.0;
}
