// iem_rmu_device.h — the kernels of the iem_rmu object (include/iem.h): the barrier parameter of the feasibility restoration phase on
// the device.  The restoration problem's dual residuals depend on mu through zeta = sqrt(mu), so its optimality error cannot be rebuilt
// for another mu from one set of words the way mu_update rebuilds E(mu); but the candidates of the monotone rule are fixed once mu is
// known — mu_{k+1} = max(mu_floor, min(kappa_mu mu_k, mu_k sqrt(mu_k))) — so rmu_error carries the two zeta-dependent maxima for all
// RMU_K candidates through ONE pass over the state, beside the words of resto_error at mu = 0 and the extremes of the complementarity
// products.  rmu_update is the rule on those 32 words, rmu_enter the start of a phase (mu_R = max(mu, max |inf|)), rmu_trigger Ipopt's
// alpha_min rule behind a search_accept, rmu_gather the one read-back's staging.  A code object of its own (no other source key knows
// of it), compiled with -ffp-contract=off behind the helpers of iem_device.h (everything in front of its own kernels, with IEM_TILE =
// 256): every line below is the order of operations of the contract in include/iem.h, each operation rounded once.
//
// NO FLOAT ATOMIC, no inline assembly and no scratch in this file: the only atomics are integer atomicMax and atomicMin on the bit
// pattern of a non-negative double, at most ONE per workgroup and slot (the scheme of res_extremes in iem_resto_device.h).  The six
// sums go through iem_shared_park / iem_shared_last / iem_shared_totals of iem_device.h as they stand — bitwise reproducible, one launch.
// The first four columns are those of resto_error, added in the order of resto_error: words 0–7 are the bits resto_error writes at
// mu = 0, zeta = zeta_0.
//
// rmu_error: the grid of the barrier object — one thread takes the entries i, i + stride, ... of [0, nvar + ncon): i < nvar is variable
// i, otherwise row j = i − nvar; flags as there.  rmu_enter, rmu_update, rmu_trigger, rmu_gather: ONE workgroup of 64 threads.

#define RMU_K 6
#define RMU_ITERATING 0ll
#define RMU_STATIONARY 1ll
#define RMU_UNUSABLE 2ll
#define RMU_INF_BITS 0x7ff0000000000000ull
#define RMU_SEARCHING 0ll
#define RMU_FAILED 3ll

// the own block, the iem_mu block, a search's control block: words of 8 bytes
enum { QW_STATUS, QW_FLAGS, QW_LAST, QW_TOTAL, QW_E0, QW_EMU, QW_MU_ENTER, QW_INF_ENTER, QW_ALPHA_MIN, QW_TRIG_ORIG, QW_TRIG_INNER };
enum { MW_MU, MW_TAU, MW_ZETA, MW_E0, MW_EMU, MW_ED, MW_EP, MW_EC0, MW_STATUS, MW_FLAGS, MW_DECREASES, MW_UPDATES };
enum { SW_ALPHA, SW_ALPHA_MAX, SW_PHI0, SW_THETA0, SW_SLOPE, SW_THETA_MIN, SW_THETA_MAX, SW_PHI_T, SW_THETA_T, SW_STATUS, SW_TRIALS, SW_COUNT, SW_FLAGS };

struct RmuArgs {
  const double *xl, *xu, *rl, *ru, *ceq;          // the barrier object's relaxed bounds and the equality rows' right-hand side
  const unsigned char *fx, *fc;
  const double *x, *s, *y, *zL, *zU, *vL, *vU;    // the state
  const double *r, *c;                            // J'y (nvar), c(x) (ncon)
  const double *p, *n_, *zp, *zn, *sR, *ws, *xR, *wx;      // the iem_resto object's vectors
  double *out;                                    // rmu_error: the 32 words; rmu_gather: the 40 words of the read-back
  const double *w;                                // rmu_update: the 32 words; rmu_enter: the 8 words of an error call
  double *blk;                                    // the own block
  double *mblk;                                   // the restoration problem's iem_mu block
  const double *oblk;                             // the ORIGINAL problem's iem_mu block, or null
  const double *rblk;                             // the iem_resto object's block
  double *ctl;                                    // rmu_trigger: the control block of the search it looks at
  double *ictl;                                   // the INNER search's control block (its filter is emptied when mu moves)
  double *alpha;                                  // rmu_trigger: d_alpha
  double *red;                                    // 6 n_wg parked values, then the ticket words
  const long long *tab;                           // offs[6] | first[6] | count[6] of iem_shared_totals
  double kappa_eps, kappa_mu, tau_min, tol, mu_floor, s_max, gamma_alpha;
  double rho, mu_host;
  double gamma_theta, gamma_phi, delta, s_theta, s_phi;      // rmu_trigger: the options of that search
  long long which;
  long long ncon, nzr;
  long long nvar, n, n_wg;
};

// np.maximum / np.minimum: a NaN in either operand gives a NaN
__device__ __forceinline__ double rmu_max(double a, double b) { return (a > b || a != a) ? a : b; }
__device__ __forceinline__ double rmu_min(double a, double b) { return (a < b || a != a) ? a : b; }
__device__ __forceinline__ double rmu_abs(double a) { return __longlong_as_double(__double_as_longlong(a) & 0x7fffffffffffffffll); }
__device__ __forceinline__ unsigned long long rmu_abs_bits(double a) { return (unsigned long long)__double_as_longlong(a) & 0x7fffffffffffffffull; }
__device__ __forceinline__ unsigned long long rmu_umin(unsigned long long a, unsigned long long b) { return a < b ? a : b; }
__device__ __forceinline__ unsigned long long rmu_umax(unsigned long long a, unsigned long long b) { return a > b ? a : b; }
__device__ __forceinline__ long long rmu_word(const double *blk, int w) { return __double_as_longlong(blk[w]); }
__device__ __forceinline__ void rmu_set_word(double *blk, int w, long long v) { blk[w] = __longlong_as_double(v); }

// the next candidate of the monotone rule
__device__ __forceinline__ double rmu_next(double mu, double kappa_mu, double mu_floor) { return rmu_max(mu_floor, rmu_min(kappa_mu * mu, mu * sqrt(mu))); }

// The extremes of the workgroup into their slots (slot s of the workgroup's NV values is word at[s] of `out`): per wave by shuffles,
// across the waves through LDS (NV·4 words), then thread s < NV holds value s of the workgroup and issues ONE integer atomic — and none
// where a relaxed agent-scope look at the slot shows that it would not change it (the slot only ever moves towards the extreme).
template <int NV, bool IS_MIN>
__device__ __forceinline__ void rmu_extremes(unsigned long long (&v)[NV], unsigned long long *out, const int (&at)[NV], unsigned long long *lds) {
  constexpr int NW = IEM_TILE / IEM_WAVE;
#pragma unroll
  for (int s = 0; s < NV; ++s) {
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long other = __shfl_xor(v[s], o, 64);
      v[s] = IS_MIN ? rmu_umin(v[s], other) : rmu_umax(v[s], other);
    }
    if (iem_lane() == 0) lds[iem_wave() * NV + s] = v[s];
  }
  __syncthreads();
  if (threadIdx.x < NV) {
    const int s = (int)threadIdx.x;
    unsigned long long b = lds[s];
    for (int w = 1; w < NW; ++w) b = IS_MIN ? rmu_umin(b, lds[w * NV + s]) : rmu_umax(b, lds[w * NV + s]);
    int word = at[0];
#pragma unroll
    for (int k = 1; k < NV; ++k) word = s == k ? at[k] : word;
    unsigned long long *slot = out + word;
    const unsigned long long cur = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (IS_MIN) { if (b < cur) atomicMin(slot, b); }
    else if (b > cur) atomicMax(slot, b);
  }
}

// one complementarity product: resto_error's maximum of |p − 0|, and mu_error's minimum over the products that are >= +0.0 (sign bit
// clear, not a NaN), sum, and count of the others
struct RmuProducts { unsigned long long mx, mn; double sum, bad; };
__device__ __forceinline__ void rmu_product(RmuProducts &q, double gap, double z) {
  const double p = gap * z;
  const unsigned long long bits = (unsigned long long)__double_as_longlong(p);
  q.mx = rmu_umax(q.mx, rmu_abs_bits(p - 0.0));
  if (bits <= RMU_INF_BITS) q.mn = rmu_umin(q.mn, bits);
  else q.bad += 1.0;
  q.sum += p;
}

extern "C" __global__ __launch_bounds__(256) void rmu_error(const RmuArgs A) {
  __shared__ double lds[32];      // 6 (NW + 1) + 1 doubles at least: the parked columns, the totals, the flag
  __shared__ unsigned long long lds_max[(4 + 2 * RMU_K) * (IEM_TILE / IEM_WAVE)];
  __shared__ unsigned long long lds_min[IEM_TILE / IEM_WAVE];
  const long long stride = (long long)gridDim.x * 256;
  const double rho = A.rho;
  // the candidates: formed once per thread
  double mu_k[RMU_K], zeta_k[RMU_K];
  mu_k[0] = A.mblk[MW_MU];
  zeta_k[0] = A.mblk[MW_ZETA];
#pragma unroll
  for (int k = 1; k < RMU_K; ++k) {
    mu_k[k] = rmu_next(mu_k[k - 1], A.kappa_mu, A.mu_floor);
    zeta_k[k] = sqrt(mu_k[k]);
  }
  unsigned long long md[RMU_K], mr[RMU_K], m2 = 0ull;
#pragma unroll
  for (int k = 0; k < RMU_K; ++k) { md[k] = 0ull; mr[k] = 0ull; }
  RmuProducts q = {0ull, RMU_INF_BITS, 0.0, 0.0};
  double v[4] = {0.0, 0.0, 0.0, 0.0};      // sum |y|, sum of the multipliers, theta_R, L: resto_error's, in its order
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < A.n; i += stride) {
    if (i < A.nvar) {
      const unsigned f = A.fx[i];
      const double x = A.x[i], wx = A.wx[i], dxr = x - A.xR[i], r = A.r[i];
      double zl = 0.0, zu = 0.0;
      if (f & 1) {
        const double d = x - A.xl[i];
        zl = A.zL[i];
        rmu_product(q, d, zl);
        v[1] += zl;
        v[3] += log(d);
      }
      if (f & 2) {
        const double d = A.xu[i] - x;
        zu = A.zU[i];
        rmu_product(q, d, zu);
        v[1] += zu;
        v[3] += log(d);
      }
#pragma unroll
      for (int k = 0; k < RMU_K; ++k) {
        const double zw = zeta_k[k] * wx;
        double t = r + zw * dxr;
        if (f & 1) t = t - zl;
        if (f & 2) t = t + zu;
        md[k] = rmu_umax(md[k], rmu_abs_bits(t));
      }
    } else {
      const long long j = i - A.nvar;
      const unsigned f = A.fc[j];
      const double y = A.y[j];
      v[0] += rmu_abs(y);
      double inf;
      if (f & 4) {
        inf = A.c[j] - A.ceq[j];
      } else {
        const double s = A.s[j], ws = A.ws[j], dsr = s - A.sR[j];
        inf = A.c[j] - s;
        double vl = 0.0, vu = 0.0;
        if (f & 1) {
          const double e = s - A.rl[j];
          vl = A.vL[j];
          rmu_product(q, e, vl);
          v[1] += vl;
          v[3] += log(e);
        }
        if (f & 2) {
          const double e = A.ru[j] - s;
          vu = A.vU[j];
          rmu_product(q, e, vu);
          v[1] += vu;
          v[3] += log(e);
        }
#pragma unroll
        for (int k = 0; k < RMU_K; ++k) {
          const double zs = zeta_k[k] * ws;
          double t = zs * dsr - y;
          if (f & 1) t = t - vl;
          if (f & 2) t = t + vu;
          mr[k] = rmu_umax(mr[k], rmu_abs_bits(t));
        }
      }
      const double p = A.p[j], n = A.n_[j], zp = A.zp[j], zn = A.zn[j];
      const unsigned long long e = rmu_umax(rmu_abs_bits((rho - y) - zp), rmu_abs_bits((rho + y) - zn));      // (no zeta in these two)
#pragma unroll
      for (int k = 0; k < RMU_K; ++k) mr[k] = rmu_umax(mr[k], e);
      const double rc = (inf - p) + n;
      m2 = rmu_umax(m2, rmu_abs_bits(rc));
      rmu_product(q, p, zp);
      rmu_product(q, n, zn);
      v[1] += zp;
      v[1] += zn;
      v[2] += rmu_abs(rc);
      v[3] += log(p);
      v[3] += log(n);
    }
  }
  // out[0..3] and the candidates' slots start from +0.0, out[8] from +inf: the 32 words were copied from the object's seed in front
  unsigned long long mx[4 + 2 * RMU_K] = {md[0], mr[0], m2, q.mx, md[0], mr[0], md[1], mr[1], md[2], mr[2], md[3], mr[3], md[4], mr[4], md[5], mr[5]}, mn[1] = {q.mn};
  static_assert(RMU_K == 6, "the slots below are those of six candidates");
  const int at_max[4 + 2 * RMU_K] = {0, 1, 2, 3, 13, 14, 16, 17, 19, 20, 22, 23, 25, 26, 28, 29}, at_min[1] = {8};
  unsigned long long *slots = reinterpret_cast<unsigned long long *>(A.out);
  rmu_extremes<4 + 2 * RMU_K, false>(mx, slots, at_max, lds_max);
  rmu_extremes<1, true>(mn, slots, at_min, lds_min);
  const double cols[6] = {v[0], v[1], v[2], v[3], q.sum, q.bad};
  iem_shared_park<6>(cols, A.red, A.tab, (long long)blockIdx.x, lds);
  if (!iem_shared_last(A.red + 6 * A.n_wg, (long long)blockIdx.x, A.n_wg, lds + 31)) return;
  iem_shared_totals(6, A.red, A.tab, A.tab + 6, A.tab + 12, lds);
  if (threadIdx.x < 4) A.out[4 + threadIdx.x] = lds[threadIdx.x];
  if (threadIdx.x == 4 || threadIdx.x == 5) A.out[5 + threadIdx.x] = lds[threadIdx.x];      // [9] the sum, [10] the count
  if (threadIdx.x == 6) {
#pragma unroll
    for (int k = 0; k < RMU_K; ++k) A.out[12 + 3 * k] = mu_k[k];
  }
}

// the inner search's filter count and flags: the 16 bytes iem_search_reset clears
__device__ __forceinline__ void rmu_empty_filter(double *ictl) { ictl[SW_COUNT] = 0.0; ictl[SW_FLAGS] = 0.0; }

// the start of a restoration phase: mu_R = max(mu, max |inf|) into the restoration block as mu_reset writes it
extern "C" __global__ __launch_bounds__(64) void rmu_enter(const RmuArgs A) {
  if (threadIdx.x != 0) return;
  const double mu_orig = A.oblk ? A.oblk[MW_MU] : A.mu_host;
  const double inf = A.w[2];
  const double mu_r = rmu_max(mu_orig, inf);
  if (!(mu_r > 0.0)) {      // a NaN or not positive: nothing else moves
    rmu_set_word(A.blk, QW_STATUS, RMU_UNUSABLE);
    return;
  }
  double *mb = A.mblk;
  mb[MW_MU] = mu_r;
  mb[MW_TAU] = rmu_max(A.tau_min, 1.0 - mu_r);
  mb[MW_ZETA] = sqrt(mu_r);
  rmu_set_word(mb, MW_STATUS, 0);
  rmu_set_word(mb, MW_FLAGS, 0);
  rmu_set_word(mb, MW_DECREASES, 0);
  rmu_set_word(mb, MW_UPDATES, 0);
  for (int k = 0; k < 16; ++k) A.blk[k] = 0.0;
  A.blk[QW_MU_ENTER] = mu_r;
  A.blk[QW_INF_ENTER] = inf;
  rmu_empty_filter(A.ictl);
}

// the restoration problem's scaled optimality error of candidate k at mu, from the 32 words
struct RmuTerms { double sd, sc, e_p; double pmax, pmin; bool has_nz; };
__device__ __forceinline__ double rmu_E(const RmuTerms &t, const double *w, int k, double mu) {
  const double e_d = rmu_max(w[13 + 3 * k], w[14 + 3 * k]) / t.sd;
  const double e_c = t.has_nz ? rmu_max(t.pmax - mu, mu - t.pmin) / t.sc : 0.0;
  return rmu_max(rmu_max(e_d, t.e_p), e_c);
}

extern "C" __global__ __launch_bounds__(64) void rmu_update(const RmuArgs A) {
  if (threadIdx.x != 0) return;
  double *blk = A.blk, *mb = A.mblk;
  const double *w = A.w;
  const double s_max = A.s_max;
  const long long m = A.ncon, nzr = A.nzr, mnz = m + nzr;
  RmuTerms t;
  t.sd = rmu_max(s_max, (w[4] + w[5]) / (double)(mnz > 1 ? mnz : 1)) / s_max;
  t.sc = rmu_max(s_max, w[5] / (double)(nzr > 1 ? nzr : 1)) / s_max;
  t.e_p = m ? w[2] : 0.0;
  t.pmax = w[3]; t.pmin = w[8];
  t.has_nz = nzr != 0;
  const double e0 = rmu_E(t, w, 0, 0.0);
  long long status, j = 0, truncated = 0;
  if (w[10] != 0.0 || e0 != e0) {
    status = RMU_UNUSABLE;
  } else if (e0 <= A.tol) {
    status = RMU_STATIONARY;
  } else {
    status = RMU_ITERATING;
    while (j < RMU_K - 1 && w[12 + 3 * j] > A.mu_floor && rmu_E(t, w, (int)j, w[12 + 3 * j]) <= A.kappa_eps * w[12 + 3 * j]) ++j;
    if (j == RMU_K - 1 && w[12 + 3 * j] > A.mu_floor && rmu_E(t, w, (int)j, w[12 + 3 * j]) <= A.kappa_eps * w[12 + 3 * j]) truncated = 2;
  }
  const double mu = w[12 + 3 * j];
  if (j > 0) {
    mb[MW_MU] = mu;
    mb[MW_TAU] = rmu_max(A.tau_min, 1.0 - mu);
    mb[MW_ZETA] = sqrt(mu);
    rmu_empty_filter(A.ictl);
  }
  rmu_set_word(blk, QW_STATUS, status);
  rmu_set_word(blk, QW_FLAGS, (j > 0 ? 1ll : 0ll) | truncated);
  rmu_set_word(blk, QW_LAST, j);
  rmu_set_word(blk, QW_TOTAL, rmu_word(blk, QW_TOTAL) + j);
  blk[QW_E0] = e0;
  blk[QW_EMU] = rmu_E(t, w, (int)j, mu);
}

// Ipopt's alpha_min behind a search_accept: a search that is still SEARCHING with its next step length below alpha_min has FAILED
extern "C" __global__ __launch_bounds__(64) void rmu_trigger(const RmuArgs A) {
  if (threadIdx.x != 0) return;
  double *ctl = A.ctl;
  if (rmu_word(ctl, SW_STATUS) != RMU_SEARCHING) return;      // decided already: nothing is written
  const double alpha = ctl[SW_ALPHA], theta0 = ctl[SW_THETA0], slope = ctl[SW_SLOPE], theta_min = ctl[SW_THETA_MIN];
  double a = A.gamma_theta;
  if (slope < 0.0) a = rmu_min(a, (A.gamma_phi * theta0) / (-slope));
  if (slope < 0.0 && theta0 <= theta_min) a = rmu_min(a, (A.delta * pow(theta0, A.s_theta)) / pow(-slope, A.s_phi));
  const double alpha_min = A.gamma_alpha * a;
  A.blk[QW_ALPHA_MIN] = alpha_min;
  if (alpha < alpha_min) {
    rmu_set_word(ctl, SW_STATUS, RMU_FAILED);
    ctl[SW_ALPHA] = 0.0;
    A.alpha[0] = 0.0;
    const int c = A.which ? QW_TRIG_INNER : QW_TRIG_ORIG;
    rmu_set_word(A.blk, c, rmu_word(A.blk, c) + 1);
  }
}

// the read-back's staging: the own block | the restoration iem_mu block | the iem_resto block, 40 words behind one another
extern "C" __global__ __launch_bounds__(64) void rmu_gather(const RmuArgs A) {
  const int l = (int)threadIdx.x;
  if (l < 16) A.out[l] = A.blk[l];
  else if (l < 32) A.out[l] = A.mblk[l - 16];
  else if (l < 40) A.out[l] = A.rblk[l - 32];
}
