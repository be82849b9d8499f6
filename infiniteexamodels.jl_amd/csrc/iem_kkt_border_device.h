// iem_kkt_border_device.h — the dense border of the chain KKT solver on the device (a code object of its own: no other source key
// knows of it; ne is a run-time argument, the LDS is dynamic).  Compiled with -ffp-contract=off: every trailing entry of the
// factorisation and every entry of a solution is produced by ONE fixed expression in a fixed order, so the bits do not depend on
// how entries are dealt to lanes — tests/border_reference.py restates both kernels operation for operation.
//
//   kkt_border_ldl     ONE workgroup.  Gs = G − gsum (gsum: the column sum of the blocks' Schur terms Gp, a device row) into LDS,
//                      then an unblocked right-looking Bunch–Kaufman LDL' with partial pivoting on the lower triangle:
//                      P Gs P' = L D L'.  Per step k: |a_kk|, the largest |a_ik| below it (lowest index on ties) by wave shuffles
//                      and one LDS exchange between the waves; the Bunch–Kaufman test (alpha = (1 + sqrt 17) / 8), for which a
//                      second maximum over row/column imax may be needed; a symmetric interchange of WHOLE rows (the columns of L
//                      already computed included); a 1 x 1 or 2 x 2 pivot; w = the scaled pivot column(s); the trailing triangle
//                      a_ij ← a_ij − a_ik w_j  or  (a_ij − a_ik w1_j) − a_ik+1 w2_j ; then w into the pivot column(s).
//                      Outputs: F (ne x ne, row-major): unit L strictly below the diagonal, D on it, the off-diagonal of a 2 x 2
//                      pivot in the subdiagonal place, zeros above; piv (ne int32), with p = the row of Gs that sits in row i of
//                      the factor:  p            a 1 x 1 pivot
//                                   −(p + 1)      the first row of a 2 x 2 pivot
//                                   −(p + 1) − ne the second row of a 2 x 2 pivot
//                      (the permutation itself, not LAPACK's interchange sequence: a solve gathers and scatters in parallel);
//                      info[0] += negative pivots, info[1] += doubtful ones (one thread, plain adds: the kernel runs behind
//                      the chain factorisation on the stream).
//                      scale = max |Gs_ij|.  A step whose diagonal entry AND column maximum are <= rel·scale (or scale == 0) is
//                      DOUBTFUL: counted, its pivot replaced by copysign(rel·scale, d), its column set to zero and nothing
//                      eliminated (do not trust the factors).  A 1 x 1 pivot counts by its sign; a 2 x 2 pivot counts one
//                      negative when its determinant is negative, by the sign of its diagonal otherwise.
//   kkt_border_solve   one workgroup per right-hand-side column u (wave 0 substitutes, the others help to load F):
//                      r = rB − sum (rB: the border entries of the right-hand side, gathered here; sum: the column sum of the
//                      blocks' terms rBp), x = P' L'^-1 D^-1 L^-1 P r: forward by columns k = 0, 1, ..., the 1 x 1 / 2 x 2 diagonal
//                      solves, backward by k = ne − 1, ..., 1 — a lane owns rows lane and lane + 64 in registers, x_k travels by
//                      a wave shuffle.  ne doubles per column where phase 1 of the chain solve reads them.  No atomics.
//   kkt_border_colsum  kkt_colsum_m's twin (csrc/iem_kkt_many_device.h) for callers without a chain module: the same partial sums
//                      in the same order.
//   kkt_border_inertia one thread: {n − negative, negative, doubtful} from the pivot counters into a device array.
//
// LDS (both kernels): ne (ne + 1) doubles of matrix (rows padded by one: a column walk is conflict-free), 2 ne + 16 doubles and
// 2 ne + 16 ints beside it — 8 (ne (ne + 1) + 2 ne + 16) + 4 (2 ne + 16) bytes: 135 360 at ne = 128.  Plain vector loads and stores.

#define KB_ALPHA 0.6403882032022076   // (1 + sqrt(17)) / 8

struct KktBorderLdlArgs {
  const double *G, *gsum;   // ne x ne each
  double *F;
  int *piv;
  long long *info;
  int ne, n_border;
  double rel;
};

// max of (v, i) over the workgroup, the lowest index on ties: shuffles inside a wave, one LDS slot per wave between them.  Every
// thread returns the same pair.  (rv, ri): a slot set of its own per use inside a step — the barrier is the only one here.
__device__ inline void kb_block_max(double &v, int &i, double *rv, int *ri) {
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(i, o, 64);
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
  }
  const int w = (int)threadIdx.x >> 6, nw = (int)blockDim.x >> 6;
  if ((threadIdx.x & 63) == 0) { rv[w] = v; ri[w] = i; }
  __syncthreads();
  v = rv[0]; i = ri[0];
  for (int q = 1; q < nw; ++q) {
    const double ov = rv[q];
    const int oi = ri[q];
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
  }
}

extern "C" __global__ __launch_bounds__(256) void kkt_border_ldl(const KktBorderLdlArgs P) {
  extern __shared__ __attribute__((aligned(16))) char kb_smem[];
  const int n = P.ne, ld = n + 1, t = (int)threadIdx.x, T = (int)blockDim.x, lane = t & 63, wv = t >> 6, nw = T >> 6;
  double *A = (double *)kb_smem, *w1 = A + n * ld, *w2 = w1 + n, *rv = w2 + n;   // rv: 16 doubles (three slot sets of four)
  int *ri = (int *)(rv + 16), *perm = ri + 16, *typ = perm + n;
  double best = -1.0;
  int bi = 0;
  for (int i = wv; i < n; i += nw)
    for (int j = lane; j < n; j += 64) {
      const double g = P.G[i * n + j] - P.gsum[i * n + j];
      A[i * ld + j] = g;
      const double a = fabs(g);
      if (a > best) best = a;
    }
  for (int i = t; i < n; i += T) { perm[i] = i; typ[i] = 0; }
  kb_block_max(best, bi, rv, ri);
  const double scale = best < 0.0 ? 0.0 : best, thr = P.rel * scale;
  long long neg = 0, dbt = 0;
  int k = 0;
  while (k < n) {      // (every quantity that steers the flow is the same in every thread: the barriers below are uniform)
    const double akk = A[k * ld + k], absakk = fabs(akk);
    double colmax = -1.0;
    int imax = 0x7fffffff;
    for (int i = k + 1 + t; i < n; i += T) {
      const double a = fabs(A[i * ld + k]);
      if (a > colmax) { colmax = a; imax = i; }
    }
    kb_block_max(colmax, imax, rv + 4, ri + 4);
    if (colmax < 0.0) { colmax = 0.0; imax = -1; }
    if (scale == 0.0 || (absakk <= thr && colmax <= thr)) {
      if (t == 0) A[k * ld + k] = copysign(thr, akk);
      for (int i = k + 1 + t; i < n; i += T) A[i * ld + k] = 0.0;
      ++dbt;
      __syncthreads();
      k += 1;
      continue;
    }
    int kp = k, kstep = 1;
    if (!(absakk >= KB_ALPHA * colmax)) {
      const double dimax = fabs(A[imax * ld + imax]);
      double rowmax = -1.0;
      int ridx = 0;
      for (int j = k + t; j < imax; j += T) {
        const double a = fabs(A[imax * ld + j]);
        if (a > rowmax) rowmax = a;
      }
      for (int i = imax + 1 + t; i < n; i += T) {
        const double a = fabs(A[i * ld + imax]);
        if (a > rowmax) rowmax = a;
      }
      kb_block_max(rowmax, ridx, rv + 8, ri + 8);
      if (absakk >= KB_ALPHA * colmax * (colmax / rowmax)) kp = k;
      else if (dimax >= KB_ALPHA * rowmax) kp = imax;
      else { kp = imax; kstep = 2; }
    }
    const int kk = k + kstep - 1;
    if (kp != kk) {      // rows / columns kk < kp of the lower triangle change places, the finished columns of L with them
      for (int j = t; j < n; j += T) {
        int a, b;
        if (j < kk) { a = kk * ld + j; b = kp * ld + j; }
        else if (j == kk) { a = kk * ld + kk; b = kp * ld + kp; }
        else if (j < kp) { a = j * ld + kk; b = kp * ld + j; }
        else if (j == kp) continue;
        else { a = j * ld + kk; b = j * ld + kp; }
        const double x = A[a];
        A[a] = A[b];
        A[b] = x;
      }
      if (t == 0) { const int x = perm[kk]; perm[kk] = perm[kp]; perm[kp] = x; }
    }
    __syncthreads();
    const int j0 = k + kstep;
    if (kstep == 1) {
      const double d = A[k * ld + k];
      if (d < 0.0) ++neg;
      for (int j = j0 + t; j < n; j += T) w1[j] = A[j * ld + k] / d;
    } else {
      const double e = A[(k + 1) * ld + k], dkk = A[k * ld + k], dk1 = A[(k + 1) * ld + k + 1];
      const double d11 = dk1 / e, d22 = dkk / e, tt = 1.0 / (d11 * d22 - 1.0), es = tt / e;
      for (int j = j0 + t; j < n; j += T) {
        const double ajk = A[j * ld + k], ajk1 = A[j * ld + k + 1];
        w1[j] = es * (d11 * ajk - ajk1);
        w2[j] = es * (d22 * ajk1 - ajk);
      }
      const double det = dkk * dk1 - e * e;
      if (det < 0.0) neg += 1;
      else if (dkk < 0.0) neg += 2;
      if (t == 0) { typ[k] = 1; typ[k + 1] = 2; }
    }
    __syncthreads();
    for (int j = j0 + wv; j < n; j += nw) {      // a wave per column, a lane per row: every entry once, by one expression
      const double wj1 = w1[j];
      if (kstep == 1) {
        for (int i = j + lane; i < n; i += 64) A[i * ld + j] = A[i * ld + j] - A[i * ld + k] * wj1;
      } else {
        const double wj2 = w2[j];
        for (int i = j + lane; i < n; i += 64) A[i * ld + j] = (A[i * ld + j] - A[i * ld + k] * wj1) - A[i * ld + k + 1] * wj2;
      }
    }
    __syncthreads();
    for (int j = j0 + t; j < n; j += T) {
      A[j * ld + k] = w1[j];
      if (kstep == 2) A[j * ld + k + 1] = w2[j];
    }
    k += kstep;
  }
  __syncthreads();
  for (int i = wv; i < n; i += nw)
    for (int j = lane; j < n; j += 64) P.F[i * n + j] = j <= i ? A[i * ld + j] : 0.0;
  for (int i = t; i < n; i += T) P.piv[i] = typ[i] == 0 ? perm[i] : typ[i] == 1 ? -(perm[i] + 1) : -(perm[i] + 1) - n;
  if (t == 0) { P.info[0] += neg; P.info[1] += dbt; }
}

struct KktBorderSolveArgs {
  const double *F;
  const int *piv;
  const double *rhs;            // column u: rhs + u ld_rhs
  const long long *src, *dst;   // r[dst[j]] = rhs[src[j]] for j < n_border (null: the identity)
  const double *sum;            // column u: sum + u ld_sum, ne doubles
  double *xB;                   // column u: xB + u ld_x, ne doubles
  long long ld_rhs, ld_sum, ld_x;
  int ne, n_border;
};

extern "C" __global__ __launch_bounds__(256) void kkt_border_solve(const KktBorderSolveArgs P) {
  extern __shared__ __attribute__((aligned(16))) char kb_smem[];
  const int n = P.ne, ld = n + 1, t = (int)threadIdx.x, T = (int)blockDim.x, lane = t & 63, wv = t >> 6, nw = T >> 6;
  const long long u = (long long)blockIdx.x;
  double *A = (double *)kb_smem, *rs = A + n * ld, *xs = rs + n;
  for (int i = wv; i < n; i += nw)
    for (int j = lane; j <= i; j += 64) A[i * ld + j] = P.F[i * n + j];
  for (int i = t; i < n; i += T) rs[i] = 0.0;
  __syncthreads();
  for (int j = t; j < P.n_border; j += T) {
    const long long d = P.dst ? P.dst[j] : j, s = P.src ? P.src[j] : j;
    if (d >= 0 && d < n) rs[d] = P.rhs[u * P.ld_rhs + s];
  }
  __syncthreads();
  for (int i = t; i < n; i += T) rs[i] = rs[i] - P.sum[u * P.ld_sum + i];
  __syncthreads();
  const int ia = lane, ib = lane + 64;      // (wave 0 only from here; the others keep the barriers company)
  int pa = ia, pb = ib, ta = 0, tb = 0;
  double xa = 0.0, xb = 0.0;
  if (t < 64) {
    if (ia < n) { int p = P.piv[ia]; if (p < 0) { p = -p - 1; ta = 1; if (p >= n) { p -= n; ta = 2; } } pa = p < n ? p : ia; }
    if (ib < n) { int p = P.piv[ib]; if (p < 0) { p = -p - 1; tb = 1; if (p >= n) { p -= n; tb = 2; } } pb = p < n ? p : ib; }
    if ((ta == 1 && ia + 1 >= n) || (ta == 2 && ia < 1)) ta = 0;      // (a malformed piv must not index outside the matrix)
    if (tb == 1 && ib + 1 >= n) tb = 0;
    if (ia < n) xa = rs[pa];
    if (ib < n) xb = rs[pb];
    for (int k = 0; k + 1 < n; ++k) {      // L z = P r by columns
      const double xk = __shfl(k < 64 ? xa : xb, k & 63, 64);
      if (ia > k && ia < n && !(ta == 2 && k == ia - 1)) xa = xa - A[ia * ld + k] * xk;
      if (ib < n && ib > k && !(tb == 2 && k == ib - 1)) xb = xb - A[ib * ld + k] * xk;
    }
    if (ia < n) xs[ia] = xa;
    if (ib < n) xs[ib] = xb;
  }
  __syncthreads();
  if (t < 64) {
    for (int h = 0; h < 2; ++h) {      // D y = z
      const int i = h ? ib : ia, ty = h ? tb : ta;
      if (i >= n) continue;
      double x;
      if (ty == 0) x = xs[i] / A[i * ld + i];
      else {
        const int i0 = ty == 1 ? i : i - 1;
        const double e = A[(i0 + 1) * ld + i0], akm1 = A[i0 * ld + i0] / e, ak = A[(i0 + 1) * ld + i0 + 1] / e, denom = akm1 * ak - 1.0;
        const double bkm1 = xs[i0] / e, bk = xs[i0 + 1] / e;
        x = ty == 1 ? (ak * bkm1 - bk) / denom : (akm1 * bk - bkm1) / denom;
      }
      if (h) xb = x; else xa = x;
    }
    for (int k = n - 1; k >= 1; --k) {      // L' x = y by columns of L', from the last
      const double xk = __shfl(k < 64 ? xa : xb, k & 63, 64);
      if (ia < k && !(ta == 1 && k == ia + 1)) xa = xa - A[k * ld + ia] * xk;
      if (ib < k && !(tb == 1 && k == ib + 1)) xb = xb - A[k * ld + ib] * xk;
    }
    if (ia < n) P.xB[u * P.ld_x + pa] = xa;
    if (ib < n) P.xB[u * P.ld_x + pb] = xb;
  }
}

struct KktBorderSumArgs { const double *in; double *out; long long rows, w, rows_per_wg, in_ld, out_ld, wgs; };
extern "C" __global__ __launch_bounds__(256) void kkt_border_colsum(const KktBorderSumArgs A) {
  const long long u = (long long)blockIdx.x / A.wgs, bx = (long long)blockIdx.x - u * A.wgs;
  const long long ncc = (A.w + 255) / 256, rc = bx / ncc, cc = bx % ncc;
  const long long c = cc * 256 + threadIdx.x;
  if (c >= A.w) return;
  const double *in = A.in + u * A.in_ld;
  const long long r0 = rc * A.rows_per_wg, r1 = r0 + A.rows_per_wg < A.rows ? r0 + A.rows_per_wg : A.rows;
  double acc = 0.0;
  for (long long r = r0; r < r1; ++r) acc += in[r * A.w + c];
  A.out[u * A.out_ld + rc * A.w + c] = acc;
}

struct KktBorderInertiaArgs { const long long *info; long long *out; long long n; };
extern "C" __global__ __launch_bounds__(64) void kkt_border_inertia(const KktBorderInertiaArgs A) {
  if (blockIdx.x == 0 && threadIdx.x == 0) { A.out[0] = A.n - A.info[0]; A.out[1] = A.info[0]; A.out[2] = A.info[1]; }
}
