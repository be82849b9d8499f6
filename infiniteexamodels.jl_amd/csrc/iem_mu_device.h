// iem_mu_device.h — the kernels of the iem_mu object (include/iem.h): the barrier parameter of a primal-dual interior-point method
// on the device — the error terms of the stopping test together with what the Fiacco–McCormick rule needs of the complementarity
// products (mu_error), and the rule itself: Ipopt's scaled optimality error at mu = 0 and at the current mu, the stopping test, the
// monotone decrease  mu <- max(floor, min(kappa_mu mu, mu sqrt(mu)))  repeated while the barrier problem counts as solved, and
// tau = max(tau_min, 1 − mu) (mu_update).  The values live in a block of sixteen 8-byte words (layout in include/iem.h) that the
// barrier, search and second-order-correction kernels read once bound.  A code object of its own (no other source key knows of it),
// compiled with -ffp-contract=off behind the helpers of iem_device.h (everything in front of its own kernels, with IEM_TILE = 256):
// every line below is the order of operations of the contract in include/iem.h, each operation rounded once.
//
// NO FLOAT ATOMIC, no inline assembly and no scratch in this file: the only atomics are integer atomicMax and atomicMin on the bit
// pattern of a non-negative double, at most ONE per workgroup and slot (the scheme of bar_extremes in iem_barrier_device.h: shuffles,
// LDS, a relaxed look at the slot).  The six sums go through iem_shared_park / iem_shared_last of iem_device.h as they stand and through
// mu_totals below, which is iem_shared_totals column for column: a lane adds its entries in index order, every workgroup parks its
// values, the workgroup that arrives last totals each column in a fixed order — bitwise reproducible, one launch.  The first four columns are those of barrier_error, added in the order
// of barrier_error: words 0–7 of mu_error are the bits barrier_error writes at mu = 0.
//
// mu_error: the grid of the barrier object — one thread takes the entries i, i + stride, ... of [0, nvar + ncon): i < nvar is variable
// i, otherwise row j = i − nvar; flags as there (fx / fc bit 0 = lower bound present, bit 1 = upper, fc bit 2 = equality row).
// mu_update, mu_reset: ONE workgroup of 64 threads, one thread decides.

#define MU_ITERATING 0ll
#define MU_CONVERGED 1ll
#define MU_UNUSABLE 2ll
#define MU_INF_BITS 0x7ff0000000000000ull
#define MU_MAX_DECREASES 64

// the block: words of 8 bytes
enum { MW_MU, MW_TAU, MW_ZETA, MW_E0, MW_EMU, MW_ED, MW_EP, MW_EC0, MW_STATUS, MW_FLAGS, MW_DECREASES, MW_UPDATES };

struct MuArgs {
  const double *xl, *xu, *rl, *ru, *ceq;          // the barrier object's relaxed bounds and the equality rows' right-hand side
  const unsigned char *fx, *fc;
  const double *x, *s, *y, *zL, *zU, *vL, *vU;    // the state
  const double *r, *c;                            // sigma grad f + J'y (nvar), c(x) (ncon)
  double *out;                                    // mu_error: the twelve words
  const double *w;                                // mu_update: the twelve words
  double *blk;                                    // the block
  double *sctl;                                   // mu_update: the control block of a search whose filter a decrease empties, or null
  double *red;                                    // 6 n_wg parked values, then the ticket words (the object's own)
  const long long *tab;                           // offs[6] | first[6] | count[6] of iem_shared_totals
  double kappa_eps, kappa_mu, tau_min, tol, mu_floor, s_max;
  double mu0;                                     // mu_reset
  long long ncon, nz;
  long long nvar, n, n_wg;
};

// np.maximum / np.minimum: a NaN in either operand gives a NaN
__device__ __forceinline__ double mu_max(double a, double b) { return (a > b || a != a) ? a : b; }
__device__ __forceinline__ double mu_min(double a, double b) { return (a < b || a != a) ? a : b; }
__device__ __forceinline__ double mu_abs(double a) { return __longlong_as_double(__double_as_longlong(a) & 0x7fffffffffffffffll); }
__device__ __forceinline__ unsigned long long mu_abs_bits(double a) { return (unsigned long long)__double_as_longlong(a) & 0x7fffffffffffffffull; }
__device__ __forceinline__ unsigned long long mu_umin(unsigned long long a, unsigned long long b) { return a < b ? a : b; }
__device__ __forceinline__ unsigned long long mu_umax(unsigned long long a, unsigned long long b) { return a > b ? a : b; }
__device__ __forceinline__ long long mu_word(const double *blk, int w) { return __double_as_longlong(blk[w]); }
__device__ __forceinline__ void mu_set_word(double *blk, int w, long long v) { blk[w] = __longlong_as_double(v); }

// The extremes of the workgroup into their slots: per wave by shuffles, across the waves through LDS (NV·4 words), then thread s < NV
// holds value s of the workgroup and issues ONE integer atomic — and none where a relaxed agent-scope look at the slot shows that it
// would not change it (the slot only ever moves towards the extreme, so a stale look can only cost an atomic, never lose a value).
template <int NV, bool IS_MIN>
__device__ __forceinline__ void mu_extremes(unsigned long long (&v)[NV], unsigned long long *slots, unsigned long long *lds) {
  constexpr int NW = IEM_TILE / IEM_WAVE;
#pragma unroll
  for (int s = 0; s < NV; ++s) {
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long other = __shfl_xor(v[s], o, 64);
      v[s] = IS_MIN ? mu_umin(v[s], other) : mu_umax(v[s], other);
    }
    if (iem_lane() == 0) lds[iem_wave() * NV + s] = v[s];
  }
  __syncthreads();
  if (threadIdx.x < NV) {
    const int s = (int)threadIdx.x;
    unsigned long long b = lds[s];
    for (int w = 1; w < NW; ++w) b = IS_MIN ? mu_umin(b, lds[w * NV + s]) : mu_umax(b, lds[w * NV + s]);
    const unsigned long long cur = __hip_atomic_load(slots + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (IS_MIN) { if (b < cur) atomicMin(slots + s, b); }
    else if (b > cur) atomicMax(slots + s, b);
  }
}

// one complementarity product: the maximum of |p| (barrier_error's  |p − 0|), the minimum over the products that are >= +0.0 (sign
// bit clear, not a NaN: exactly the bit patterns up to +inf), the sum, and the count of the others
struct MuProducts { unsigned long long mx, mn; double sum, bad; };
__device__ __forceinline__ void mu_product(MuProducts &q, double gap, double z) {
  const double p = gap * z;
  const unsigned long long bits = (unsigned long long)__double_as_longlong(p);
  q.mx = mu_umax(q.mx, mu_abs_bits(p));
  if (bits <= MU_INF_BITS) q.mn = mu_umin(q.mn, bits);
  else q.bad += 1.0;
  q.sum += p;
}

// iem_shared_totals for the six columns, column for column in ITS order — lane l adds the entries l, l + 64, ... one after the other
// from +0.0, then iem_wave_sum — so every total carries the bits iem_shared_totals gives; but wave w takes its two columns w and w + 4
// in ONE loop and loads four entries of each ahead of their additions, so that a lane's loads do not wait for one another: this loop
// is the tail of the launch, and with one column after the other it was a third of mu_error at 4096 workgroups
__device__ __forceinline__ void mu_totals(const double *__restrict__ red, const long long *__restrict__ offs, const long long *__restrict__ first,
                                          const long long *__restrict__ count, double *__restrict__ lds) {
  constexpr int NW = IEM_TILE / IEM_WAVE;
  static_assert(NW == 4, "six columns over four waves: waves 0 and 1 take two");
  const int w = iem_wave(), l = iem_lane();
  const bool two = w + NW < 6;
  const double *__restrict__ ca = red + offs[w] + first[w];
  const double *__restrict__ cb = two ? red + offs[w + NW] + first[w + NW] : ca;
  const long long na = count[w], nb = two ? count[w + NW] : 0;
  const long long nmax = na > nb ? na : nb;
  double a = 0.0, b = 0.0;
  for (long long i = l; i < nmax; i += 4 * IEM_WAVE) {
    double va[4], vb[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long long j = i + u * IEM_WAVE;
      va[u] = j < na ? __hip_atomic_load(ca + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
      vb[u] = j < nb ? __hip_atomic_load(cb + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long long j = i + u * IEM_WAVE;
      if (j < na) a += va[u];
      if (j < nb) b += vb[u];
    }
  }
  a = iem_wave_sum(a);
  b = iem_wave_sum(b);
  if (l == 0) {
    lds[w] = a;
    if (two) lds[w + NW] = b;
  }
  __syncthreads();
}

extern "C" __global__ __launch_bounds__(256) void mu_error(const MuArgs A) {
  __shared__ double lds[32];      // 6 (NW + 1) + 1 doubles at least: the parked columns, the totals, the flag
  __shared__ unsigned long long lds_max[4 * (IEM_TILE / IEM_WAVE)];
  __shared__ unsigned long long lds_min[IEM_TILE / IEM_WAVE];
  const long long stride = (long long)gridDim.x * 256;
  unsigned long long m0 = 0ull, m1 = 0ull, m2 = 0ull;
  MuProducts q = {0ull, MU_INF_BITS, 0.0, 0.0};
  double v[4] = {0.0, 0.0, 0.0, 0.0};      // sum |y|, sum of the present multipliers, theta, sum log gap: barrier_error's, in its order
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < A.n; i += stride) {
    if (i < A.nvar) {
      const unsigned f = A.fx[i];
      const double x = A.x[i];
      double t = A.r[i];
      if (f & 1) {
        const double d = x - A.xl[i], z = A.zL[i];
        t = t - z;
        mu_product(q, d, z);
        v[1] += z;
        v[3] += log(d);
      }
      if (f & 2) {
        const double d = A.xu[i] - x, z = A.zU[i];
        t = t + z;
        mu_product(q, d, z);
        v[1] += z;
        v[3] += log(d);
      }
      m0 = mu_umax(m0, mu_abs_bits(t));
    } else {
      const long long j = i - A.nvar;
      const unsigned f = A.fc[j];
      const double y = A.y[j];
      v[0] += mu_abs(y);
      double inf;
      if (f & 4) {
        inf = A.c[j] - A.ceq[j];
      } else {
        const double s = A.s[j];
        inf = A.c[j] - s;
        double t = -y;
        if (f & 1) {
          const double e = s - A.rl[j], z = A.vL[j];
          t = t - z;
          mu_product(q, e, z);
          v[1] += z;
          v[3] += log(e);
        }
        if (f & 2) {
          const double e = A.ru[j] - s, z = A.vU[j];
          t = t + z;
          mu_product(q, e, z);
          v[1] += z;
          v[3] += log(e);
        }
        m1 = mu_umax(m1, mu_abs_bits(t));
      }
      m2 = mu_umax(m2, mu_abs_bits(inf));
      v[2] += mu_abs(inf);
    }
  }
  // out[0..3] start from +0.0, out[8] from +inf, out[11] is +0.0: the twelve words were copied from the object's seed in front
  unsigned long long mx[4] = {m0, m1, m2, q.mx}, mn[1] = {q.mn};
  unsigned long long *slots = reinterpret_cast<unsigned long long *>(A.out);
  mu_extremes<4, false>(mx, slots, lds_max);
  mu_extremes<1, true>(mn, slots + 8, lds_min);
  const double cols[6] = {v[0], v[1], v[2], v[3], q.sum, q.bad};
  iem_shared_park<6>(cols, A.red, A.tab, (long long)blockIdx.x, lds);
  if (!iem_shared_last(A.red + 6 * A.n_wg, (long long)blockIdx.x, A.n_wg, lds + 31)) return;
  mu_totals(A.red, A.tab, A.tab + 6, A.tab + 12, lds);
  if (threadIdx.x < 4) A.out[4 + threadIdx.x] = lds[threadIdx.x];
  if (threadIdx.x == 4 || threadIdx.x == 5) A.out[5 + threadIdx.x] = lds[threadIdx.x];      // [9] the sum, [10] the count
}

// a new solve: words 0–2 from mu0, status ITERATING, flags and counters 0; words 3–7 stay
extern "C" __global__ __launch_bounds__(64) void mu_reset(const MuArgs A) {
  if (threadIdx.x != 0) return;
  double *blk = A.blk;
  blk[MW_MU] = A.mu0;
  blk[MW_TAU] = mu_max(A.tau_min, 1.0 - A.mu0);
  blk[MW_ZETA] = sqrt(A.mu0);
  mu_set_word(blk, MW_STATUS, MU_ITERATING);
  mu_set_word(blk, MW_FLAGS, 0);
  mu_set_word(blk, MW_DECREASES, 0);
  mu_set_word(blk, MW_UPDATES, 0);
}

// Ipopt's scaled optimality error from the twelve words: e_d, e_p, and the complementarity term as a function of mu
struct MuTerms { double e_d, e_p, sc; double pmax, pmin; bool has_nz; };
__device__ __forceinline__ double mu_ec(const MuTerms &t, double mu) { return t.has_nz ? mu_max(t.pmax - mu, mu - t.pmin) / t.sc : 0.0; }
__device__ __forceinline__ double mu_E(const MuTerms &t, double mu) { return mu_max(mu_max(t.e_d, t.e_p), mu_ec(t, mu)); }

extern "C" __global__ __launch_bounds__(64) void mu_update(const MuArgs A) {
  if (threadIdx.x != 0) return;
  double *blk = A.blk;
  const double *w = A.w;
  const double s_max = A.s_max;
  const long long m = A.ncon, nz = A.nz, mnz = m + nz;
  const double sd = mu_max(s_max, (w[4] + w[5]) / (double)(mnz > 1 ? mnz : 1)) / s_max;
  MuTerms t;
  t.sc = mu_max(s_max, w[5] / (double)(nz > 1 ? nz : 1)) / s_max;
  t.e_d = mu_max(w[0], w[1]) / sd;
  t.e_p = m ? w[2] : 0.0;
  t.pmax = w[3]; t.pmin = w[8];
  t.has_nz = nz != 0;
  double mu = blk[MW_MU];
  const double e0 = mu_E(t, 0.0), ec0 = mu_ec(t, 0.0);
  long long status, k = 0;
  if (w[10] != 0.0 || e0 != e0) {
    status = MU_UNUSABLE;
  } else if (e0 <= A.tol) {
    status = MU_CONVERGED;
  } else {
    status = MU_ITERATING;
    while (mu > A.mu_floor && mu_E(t, mu) <= A.kappa_eps * mu && k < MU_MAX_DECREASES) {
      mu = mu_max(A.mu_floor, mu_min(A.kappa_mu * mu, mu * sqrt(mu)));
      ++k;
    }
  }
  const long long flags = mu_word(blk, MW_FLAGS);
  if (k > 0) {
    blk[MW_MU] = mu;
    blk[MW_TAU] = mu_max(A.tau_min, 1.0 - mu);
    blk[MW_ZETA] = sqrt(mu);
    mu_set_word(blk, MW_FLAGS, flags | 1ll);
    mu_set_word(blk, MW_DECREASES, mu_word(blk, MW_DECREASES) + k);
    if (A.sctl) { A.sctl[11] = 0.0; A.sctl[12] = 0.0; }      // the filter count and the flags: what iem_search_reset clears
  } else {
    mu_set_word(blk, MW_FLAGS, flags & ~1ll);
  }
  blk[MW_E0] = e0;
  blk[MW_EMU] = mu_E(t, mu);
  blk[MW_ED] = t.e_d;
  blk[MW_EP] = t.e_p;
  blk[MW_EC0] = ec0;
  mu_set_word(blk, MW_STATUS, status);
  mu_set_word(blk, MW_UPDATES, mu_word(blk, MW_UPDATES) + 1);
}
