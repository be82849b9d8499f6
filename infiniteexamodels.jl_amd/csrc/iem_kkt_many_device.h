// iem_kkt_many_device.h — the chain KKT solver's SOLVE kernels for several right-hand sides at once (iem_kkt_solve_many /
// iem_kkt_chain_solve_many).  Appended behind iem_kkt_device.h in every chain KKT code object (kkt_source, csrc/iem_api.cpp).
//
// The single-column solves (kkt_forward / kkt_backward, kkt_fz / kkt_fs / kkt_bw) are matrix-vector work: every level streams
// the block inverses D^-1 and the couplings Bt, BR, Z through HBM for ONE vector — 1.5 GB of factors next to 64 MB of vectors at
// 1e5 quadrotor supports.  The kernels here load every entry of a factor ONCE and apply it to a chunk of KKT_MR columns:
// KKT_MR accumulators per lane in registers, the chunk's vectors side by side in LDS.
//
// Layout of a chunk: column u of r / z sits at  r + u * S * NB  (rBp: + u * S * NE, xB: + u * NE) — PLANES, not interleaved.
// Every global access of a column is then the access the single-column kernel makes (same coalescing), and in LDS column u
// of a vector is v[u * NB + k]: whatever the lanes read of ONE column is what the single-column kernel reads of its vector
// (a broadcast, or consecutive doubles), so the column index never enters the bank pattern — an interleaved v[k * MR + u]
// with MR a power of two would put the columns of neighbouring k into the same banks.
//
// CONTRACT: per column, the operations of the single-column kernel of the same family in the same order (the same
// summation order over k, the same shuffle tree in kkt_forward) — column u of a chunk is bit for bit what the single-column
// solve gives for it, whatever KKT_MR is, wherever the column sits in the chunk, whatever the other columns hold.  (The code
// objects are compiled with -ffp-contract=off unless the experiment knob says otherwise: a product and a sum are two
// roundings in both forms.)  Columns nr .. KKT_MR - 1 of a remainder chunk are computed on zeros and never stored.
#ifndef IEM_KKT_MANY_DEVICE_H
#define IEM_KKT_MANY_DEVICE_H

#ifndef KKT_MR
#define KKT_MR 4                  // columns per chunk (host-chosen per shape: kkt_many_width in csrc/iem_api.cpp)
#endif

struct KktSolveManyArgs {
  const double *D, *Bt, *BR, *Z;   // as KktSolveArgs
  const int *rows, *cols;
  double *r;                     // MR planes of S x NB: right-hand sides in, solutions out
  double *z;                     // MR planes of S x NB
  double *rBp;                   // MR planes of S x NE
  const double *xB;              // MR x NE
  long long S, s;
  int final_block;
  long long T;
  int nr;                        // columns of this chunk, 1 .. KKT_MR
};

// acc[u] = sum_k M[k][c] * v[u][k]   (kkt_tdot per column; M[k][c] loaded once)
__device__ __forceinline__ void kkt_tdot_m(double (&acc)[KKT_MR], const double *__restrict__ M, const double *v, int cols, int c) {
#pragma unroll
  for (int u = 0; u < KKT_MR; ++u) acc[u] = 0.0;
#pragma unroll 4
  for (int k = 0; k < KKT_NB; ++k) {
    const double d = M[(long long)k * cols + c];
#pragma unroll
    for (int u = 0; u < KKT_MR; ++u) acc[u] += d * v[u * KKT_NB + k];
  }
}

// ---- the 64-thread family ------------------------------------------------------------------------------------------------
extern "C" __global__ __launch_bounds__(64) void kkt_forward_m(const KktSolveManyArgs A) {
  __shared__ double v[KKT_MR * KKT_NB], zc[KKT_MR * KKT_NC], zr[KKT_MR * KKT_NC];
  __shared__ int rr[KKT_NC], cc[KKT_NC];
  const long long T_ = A.T > 0 ? A.T : A.S;
  const long long n_surv = A.final_block ? 0 : (A.S / T_) * ((T_ + 2 * A.s - 1) / (2 * A.s));
  const long long pl = A.S * KKT_NB;
  const int t = (int)threadIdx.x, nr = A.nr;
  constexpr int NN = KKT_NC * KKT_NC;
  if ((long long)blockIdx.x < n_surv) {
    const KktIdx jx = kkt_survivor((long long)blockIdx.x, A.s, A.S, A.T);
    const long long j = jx.i, p = j - A.s, q = j + A.s;
    const bool hp = jx.left, hq = jx.right;
    for (int e = t; e < KKT_NC; e += 64) {
      rr[e] = A.rows[e]; cc[e] = A.cols[e];
#pragma unroll
      for (int u = 0; u < KKT_MR; ++u) { zc[u * KKT_NC + e] = 0.0; zr[u * KKT_NC + e] = 0.0; }
    }
    if (hp) {
      for (int e = t; e < KKT_NB; e += 64) {
#pragma unroll
        for (int u = 0; u < KKT_MR; ++u) v[u * KKT_NB + e] = u < nr ? A.r[u * pl + p * KKT_NB + e] : 0.0;
      }
      __syncthreads();
      for (int a0 = 0; a0 < KKT_NC; a0 += 16) {
        const int a = a0 + (t >> 2);
        double acc[KKT_MR];
#pragma unroll
        for (int u = 0; u < KKT_MR; ++u) acc[u] = 0.0;
        if (a < KKT_NC && cc[a] >= 0) {
          const double *row = A.D + (p * KKT_NB + cc[a]) * KKT_NB;
#pragma unroll 2
          for (int k = t & 3; k < KKT_NB; k += 4) {
            const double d = row[k];
#pragma unroll
            for (int u = 0; u < KKT_MR; ++u) acc[u] += d * v[u * KKT_NB + k];
          }
        }
#pragma unroll
        for (int u = 0; u < KKT_MR; ++u) { acc[u] += __shfl_xor(acc[u], 1); acc[u] += __shfl_xor(acc[u], 2); }
        if (a < KKT_NC && (t & 3) == 0) {
#pragma unroll
          for (int u = 0; u < KKT_MR; ++u) zc[u * KKT_NC + a] = acc[u];
        }
      }
      __syncthreads();
    }
    if (hq) {
      for (int e = t; e < KKT_NB; e += 64) {
#pragma unroll
        for (int u = 0; u < KKT_MR; ++u) v[u * KKT_NB + e] = u < nr ? A.r[u * pl + q * KKT_NB + e] : 0.0;
      }
      __syncthreads();
      for (int a0 = 0; a0 < KKT_NC; a0 += 16) {
        const int a = a0 + (t >> 2);
        double acc[KKT_MR];
#pragma unroll
        for (int u = 0; u < KKT_MR; ++u) acc[u] = 0.0;
        if (a < KKT_NC && rr[a] >= 0) {
          const double *row = A.D + (q * KKT_NB + rr[a]) * KKT_NB;
#pragma unroll 2
          for (int k = t & 3; k < KKT_NB; k += 4) {
            const double d = row[k];
#pragma unroll
            for (int u = 0; u < KKT_MR; ++u) acc[u] += d * v[u * KKT_NB + k];
          }
        }
#pragma unroll
        for (int u = 0; u < KKT_MR; ++u) { acc[u] += __shfl_xor(acc[u], 1); acc[u] += __shfl_xor(acc[u], 2); }
        if (a < KKT_NC && (t & 3) == 0) {
#pragma unroll
          for (int u = 0; u < KKT_MR; ++u) zr[u * KKT_NC + a] = acc[u];
        }
      }
    }
    __syncthreads();
    if (hp)
      for (int a = t; a < KKT_NC; a += 64) {
        if (rr[a] < 0) continue;
        double acc[KKT_MR];
#pragma unroll
        for (int u = 0; u < KKT_MR; ++u) acc[u] = 0.0;
        for (int c = 0; c < KKT_NC; ++c) {
          const double b = A.BR[p * NN + a * KKT_NC + c];
#pragma unroll
          for (int u = 0; u < KKT_MR; ++u) acc[u] += b * zc[u * KKT_NC + c];
        }
#pragma unroll
        for (int u = 0; u < KKT_MR; ++u) if (u < nr) A.r[u * pl + j * KKT_NB + rr[a]] -= acc[u];
      }
    __threadfence_block();
    __syncthreads();
    if (hq)
      for (int a = t; a < KKT_NC; a += 64) {
        if (cc[a] < 0) continue;
        double acc[KKT_MR];
#pragma unroll
        for (int u = 0; u < KKT_MR; ++u) acc[u] = 0.0;
        for (int k = 0; k < KKT_NC; ++k) {
          const double b = A.Bt[q * NN + k * KKT_NC + a];
#pragma unroll
          for (int u = 0; u < KKT_MR; ++u) acc[u] += b * zr[u * KKT_NC + k];
        }
#pragma unroll
        for (int u = 0; u < KKT_MR; ++u) if (u < nr) A.r[u * pl + j * KKT_NB + cc[a]] -= acc[u];
      }
    return;
  }
  const long long e_idx = (long long)blockIdx.x - n_surv;
  const KktIdx ix = kkt_eliminated(e_idx, A.s, A.S, A.T);
  const long long i = A.final_block == 2 ? e_idx : A.final_block ? kkt_lane_first(e_idx, A.S, A.T) : ix.i;
  if (i >= A.S || (!A.final_block && !ix.valid)) return;
  for (int e = t; e < KKT_NB; e += 64) {
#pragma unroll
    for (int u = 0; u < KKT_MR; ++u) v[u * KKT_NB + e] = u < nr ? A.r[u * pl + i * KKT_NB + e] : 0.0;
  }
  __syncthreads();
  if (!A.final_block)
    for (int c = t; c < KKT_NB; c += 64) {
      double acc[KKT_MR];
      kkt_tdot_m(acc, A.D + i * KKT_NB * KKT_NB, v, KKT_NB, c);
#pragma unroll
      for (int u = 0; u < KKT_MR; ++u) if (u < nr) A.z[u * pl + i * KKT_NB + c] = acc[u];
    }
#if KKT_NE > 0
  for (int c = t; c < KKT_NE; c += 64) {
    double acc[KKT_MR];
    kkt_tdot_m(acc, A.Z + i * KKT_NB * KKT_NE, v, KKT_NE, c);
#pragma unroll
    for (int u = 0; u < KKT_MR; ++u) if (u < nr) A.rBp[u * A.S * KKT_NE + i * KKT_NE + c] = acc[u];
  }
#endif
}

extern "C" __global__ __launch_bounds__(64) void kkt_backward_m(const KktSolveManyArgs A) {
  __shared__ double ri[KKT_MR * KKT_NB], xc[KKT_MR * KKT_NC], xr[KKT_MR * KKT_NC], t1[KKT_MR * KKT_NC], t2[KKT_MR * KKT_NC],
      xb[KKT_MR * (KKT_NE > 0 ? KKT_NE : 1)];
  __shared__ int rr[KKT_NC], cc[KKT_NC];
  const KktIdx ix = kkt_eliminated((long long)blockIdx.x, A.s, A.S, A.T);
  const long long i = A.final_block == 2 ? (long long)blockIdx.x : A.final_block ? kkt_lane_first((long long)blockIdx.x, A.S, A.T) : ix.i;
  if (i >= A.S || (!A.final_block && !ix.valid)) return;
  const long long pl = A.S * KKT_NB;
  const int t = (int)threadIdx.x, nr = A.nr;
  constexpr int NN = KKT_NC * KKT_NC;
  const bool hp = !A.final_block, hq = !A.final_block && ix.right;
  for (int e = t; e < KKT_NC; e += 64) {
    const int re = hp ? A.rows[e] : -1, ce = hp ? A.cols[e] : -1;
    rr[e] = re; cc[e] = ce;
#pragma unroll
    for (int u = 0; u < KKT_MR; ++u) {
      xc[u * KKT_NC + e] = (hp && ce >= 0 && u < nr) ? A.r[u * pl + (i - A.s) * KKT_NB + ce] : 0.0;
      xr[u * KKT_NC + e] = (hq && re >= 0 && u < nr) ? A.r[u * pl + (i + A.s) * KKT_NB + re] : 0.0;
    }
  }
  if (A.final_block)
    for (int e = t; e < KKT_NB; e += 64) {
#pragma unroll
      for (int u = 0; u < KKT_MR; ++u) ri[u * KKT_NB + e] = u < nr ? A.r[u * pl + i * KKT_NB + e] : 0.0;
    }
#if KKT_NE > 0
  for (int e = t; e < KKT_NE; e += 64) {
#pragma unroll
    for (int u = 0; u < KKT_MR; ++u) xb[u * KKT_NE + e] = u < nr ? A.xB[u * KKT_NE + e] : 0.0;
  }
#endif
  __syncthreads();
  for (int a = t; a < KKT_NC; a += 64) {
    double s1[KKT_MR], s2[KKT_MR];
#pragma unroll
    for (int u = 0; u < KKT_MR; ++u) { s1[u] = 0.0; s2[u] = 0.0; }
    if (hp)
      for (int c = 0; c < KKT_NC; ++c) {
        const double b = A.Bt[i * NN + a * KKT_NC + c];
#pragma unroll
        for (int u = 0; u < KKT_MR; ++u) s1[u] += b * xc[u * KKT_NC + c];
      }
    if (hq)
      for (int k = 0; k < KKT_NC; ++k) {
        const double b = A.BR[i * NN + k * KKT_NC + a];
#pragma unroll
        for (int u = 0; u < KKT_MR; ++u) s2[u] += b * xr[u * KKT_NC + k];
      }
#pragma unroll
    for (int u = 0; u < KKT_MR; ++u) { t1[u * KKT_NC + a] = s1[u]; t2[u * KKT_NC + a] = s2[u]; }
  }
  __syncthreads();
  const double *Di = A.D + i * KKT_NB * KKT_NB;
  constexpr int NOUT = (KKT_NB + 63) / 64;
  double out[NOUT][KKT_MR];
#pragma unroll
  for (int n = 0; n < NOUT; ++n) {
    const int c = t + 64 * n;
#pragma unroll
    for (int u = 0; u < KKT_MR; ++u) out[n][u] = 0.0;
    if (c >= KKT_NB) continue;
    double acc[KKT_MR];
    if (A.final_block) kkt_tdot_m(acc, Di, ri, KKT_NB, c);
    else {
#pragma unroll
      for (int u = 0; u < KKT_MR; ++u) acc[u] = u < nr ? A.z[u * pl + i * KKT_NB + c] : 0.0;
    }
    if (hp)
      for (int a = 0; a < KKT_NC; ++a)
        if (rr[a] >= 0) {
          const double d = Di[rr[a] * KKT_NB + c];
#pragma unroll
          for (int u = 0; u < KKT_MR; ++u) acc[u] -= d * t1[u * KKT_NC + a];
        }
    if (hq)
      for (int a = 0; a < KKT_NC; ++a)
        if (cc[a] >= 0) {
          const double d = Di[cc[a] * KKT_NB + c];
#pragma unroll
          for (int u = 0; u < KKT_MR; ++u) acc[u] -= d * t2[u * KKT_NC + a];
        }
#if KKT_NE > 0
    {
      const double *Zr = A.Z + (i * KKT_NB + c) * KKT_NE;
      for (int e = 0; e < KKT_NE; ++e) {
        const double zz = Zr[e];
#pragma unroll
        for (int u = 0; u < KKT_MR; ++u) acc[u] -= zz * xb[u * KKT_NE + e];
      }
    }
#endif
#pragma unroll
    for (int u = 0; u < KKT_MR; ++u) out[n][u] = acc[u];
  }
#pragma unroll
  for (int n = 0; n < NOUT; ++n) {
    const int c = t + 64 * n;
    if (c < KKT_NB) {
#pragma unroll
      for (int u = 0; u < KKT_MR; ++u) if (u < nr) A.r[u * pl + i * KKT_NB + c] = out[n][u];
    }
  }
}

#if KKT_NE == 0 && KKT_NB <= 64
// ---- the lane-per-row family (no border, blocks that fit a wave) -------------------------------------------------------------
#define KKT_MRV (KKT_SBPW * KKT_NB)      // LDS doubles of one column's vectors in kkt_fz_m
extern "C" __global__ __launch_bounds__(64) void kkt_fz_m(const KktSolveManyArgs A) {
  __shared__ double rv[KKT_MR * KKT_MRV];
  const int lane = (int)threadIdx.x, slot = lane / KKT_NB, li = lane - slot * KKT_NB, nr = A.nr;
  const long long b = (long long)blockIdx.x * KKT_SBPW + slot, pl = A.S * KKT_NB;
  const KktIdx ix = kkt_eliminated(b, A.s, A.S, A.T);
  const long long i = A.final_block == 2 ? b : A.final_block ? kkt_lane_first(b, A.S, A.T) : ix.i;
  const bool on = slot < KKT_SBPW && i < A.S && (A.final_block || ix.valid);
  if (slot < KKT_SBPW) {
#pragma unroll
    for (int u = 0; u < KKT_MR; ++u) rv[u * KKT_MRV + slot * KKT_NB + li] = (on && u < nr) ? A.r[u * pl + i * KKT_NB + li] : 0.0;
  }
  __syncthreads();
  if (!on) return;
  const double *col = A.D + i * KKT_NB * KKT_NB + li, *v = rv + slot * KKT_NB;
  double acc[KKT_MR];
#pragma unroll
  for (int u = 0; u < KKT_MR; ++u) acc[u] = 0.0;
#pragma unroll 8
  for (int kk = 0; kk < KKT_NB; ++kk) {
    const double d = col[kk * KKT_NB];
#pragma unroll
    for (int u = 0; u < KKT_MR; ++u) acc[u] += d * v[u * KKT_MRV + kk];
  }
  double *o = A.final_block ? A.r : A.z;
#pragma unroll
  for (int u = 0; u < KKT_MR; ++u) if (u < nr) o[u * pl + i * KKT_NB + li] = acc[u];
}
extern "C" __global__ __launch_bounds__(64) void kkt_fs_m(const KktSolveManyArgs A) {
  const long long T_ = A.T > 0 ? A.T : A.S, n_surv = (A.S / T_) * ((T_ + 2 * A.s - 1) / (2 * A.s));
  const long long g = (long long)blockIdx.x * 64 + threadIdx.x, pl = A.S * KKT_NB;
  if (g >= n_surv) return;
  const KktIdx jx = kkt_survivor(g, A.s, A.S, A.T);
  if (!jx.valid) return;
  const long long j = jx.i, p = j - A.s, q = j + A.s;
  const int nr = A.nr;
  constexpr int NN = KKT_NC * KKT_NC;
  double zv[KKT_MR][KKT_NC];
  if (jx.left) {
#pragma unroll
    for (int c = 0; c < KKT_NC; ++c) {
      const int cc = A.cols[c];
#pragma unroll
      for (int u = 0; u < KKT_MR; ++u) zv[u][c] = (cc >= 0 && u < nr) ? A.z[u * pl + p * KKT_NB + cc] : 0.0;
    }
    for (int a = 0; a < KKT_NC; ++a) {
      const int ra = A.rows[a];
      if (ra < 0) continue;
      double acc[KKT_MR];
#pragma unroll
      for (int u = 0; u < KKT_MR; ++u) acc[u] = 0.0;
#pragma unroll
      for (int c = 0; c < KKT_NC; ++c) {
        const double br = A.BR[p * NN + a * KKT_NC + c];
#pragma unroll
        for (int u = 0; u < KKT_MR; ++u) acc[u] += br * zv[u][c];
      }
#pragma unroll
      for (int u = 0; u < KKT_MR; ++u) if (u < nr) A.r[u * pl + j * KKT_NB + ra] -= acc[u];
    }
  }
  if (jx.right) {      // (after the left half: R and C may share an entry of r_j)
#pragma unroll
    for (int c = 0; c < KKT_NC; ++c) {
      const int rr = A.rows[c];
#pragma unroll
      for (int u = 0; u < KKT_MR; ++u) zv[u][c] = (rr >= 0 && u < nr) ? A.z[u * pl + q * KKT_NB + rr] : 0.0;
    }
    for (int a = 0; a < KKT_NC; ++a) {
      const int ca = A.cols[a];
      if (ca < 0) continue;
      double acc[KKT_MR];
#pragma unroll
      for (int u = 0; u < KKT_MR; ++u) acc[u] = 0.0;
#pragma unroll
      for (int kk = 0; kk < KKT_NC; ++kk) {
        const double bt = A.Bt[q * NN + kk * KKT_NC + a];
#pragma unroll
        for (int u = 0; u < KKT_MR; ++u) acc[u] += bt * zv[u][kk];
      }
#pragma unroll
      for (int u = 0; u < KKT_MR; ++u) if (u < nr) A.r[u * pl + j * KKT_NB + ca] -= acc[u];
    }
  }
}
extern "C" __global__ __launch_bounds__(64) void kkt_bw_m(const KktSolveManyArgs A) {
  __shared__ double t1s[KKT_MR * KKT_SBPW * KKT_NC], t2s[KKT_MR * KKT_SBPW * KKT_NC];
  const int lane = (int)threadIdx.x, slot = lane / KKT_NB, li = lane - slot * KKT_NB, nr = A.nr;
  const long long b = (long long)blockIdx.x * KKT_SBPW + slot, pl = A.S * KKT_NB;
  const KktIdx ix = kkt_eliminated(b, A.s, A.S, A.T);
  const long long i = ix.i;
  const bool on = slot < KKT_SBPW && ix.valid && i < A.S;
  constexpr int NN = KKT_NC * KKT_NC, TS = KKT_SBPW * KKT_NC;
  if (on && li < KKT_NC) {
    double s1[KKT_MR], s2[KKT_MR];
#pragma unroll
    for (int u = 0; u < KKT_MR; ++u) { s1[u] = 0.0; s2[u] = 0.0; }
    for (int c = 0; c < KKT_NC; ++c) {
      const int cc = A.cols[c], rr = A.rows[c];
      if (cc >= 0) {
        const double bt = A.Bt[i * NN + li * KKT_NC + c];
#pragma unroll
        for (int u = 0; u < KKT_MR; ++u) s1[u] += bt * (u < nr ? A.r[u * pl + (i - A.s) * KKT_NB + cc] : 0.0);
      }
      if (ix.right && rr >= 0) {
        const double br = A.BR[i * NN + c * KKT_NC + li];
#pragma unroll
        for (int u = 0; u < KKT_MR; ++u) s2[u] += br * (u < nr ? A.r[u * pl + (i + A.s) * KKT_NB + rr] : 0.0);
      }
    }
#pragma unroll
    for (int u = 0; u < KKT_MR; ++u) { t1s[u * TS + slot * KKT_NC + li] = s1[u]; t2s[u * TS + slot * KKT_NC + li] = s2[u]; }
  }
  __syncthreads();
  if (!on) return;
  const double *col = A.D + i * KKT_NB * KKT_NB + li;
  double acc[KKT_MR];
#pragma unroll
  for (int u = 0; u < KKT_MR; ++u) acc[u] = u < nr ? A.z[u * pl + i * KKT_NB + li] : 0.0;
#pragma unroll
  for (int a = 0; a < KKT_NC; ++a) {
    const int ra = A.rows[a], ca = A.cols[a];
    if (ra >= 0) {
      const double d = col[ra * KKT_NB];
#pragma unroll
      for (int u = 0; u < KKT_MR; ++u) acc[u] -= d * t1s[u * TS + slot * KKT_NC + a];
    }
    if (ca >= 0) {
      const double d = col[ca * KKT_NB];
#pragma unroll
      for (int u = 0; u < KKT_MR; ++u) acc[u] -= d * t2s[u * TS + slot * KKT_NC + a];
    }
  }
#pragma unroll
  for (int u = 0; u < KKT_MR; ++u) if (u < nr) A.r[u * pl + i * KKT_NB + li] = acc[u];
}
#endif

// ---- right-hand sides in and out, border terms ---------------------------------------------------------------------------------
// Right-hand sides into the chain's block order (and the border's) and the solutions back:  dst[di[i] + u ldd] = src[si[i] + u lds]
// for the nr columns of a chunk — a thread per index pair, loaded once for all columns
struct KktMoveManyArgs { double *dst; const double *src; const long long *di, *si; long long n, ldd, lds; int nr; };
extern "C" __global__ __launch_bounds__(256) void kkt_move_m(const KktMoveManyArgs A) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= A.n) return;
  const long long d = A.di[i], s = A.si[i];
  for (int u = 0; u < A.nr; ++u) A.dst[d + u * A.ldd] = A.src[s + u * A.lds];
}
// Column sums of `rows x w` matrices (the per-block border terms), one matrix per column of a chunk: matrix u sits at in + u in_ld
// and is served by the workgroups [u wgs, (u + 1) wgs).  Workgroup b of a matrix sums the rows of chunk b / ncc (rows_per_wg rows,
// from 0.0 in row order) for the 256 columns of chunk b % ncc (ncc = ceil(w / 256)) into out[u out_ld + chunk w + column]; a second
// launch over the partials leaves one row (kkt_border_sums in csrc/iem_api.cpp).  The order of the additions is fixed: the sums are
// bitwise reproducible, and kkt_border_colsum (csrc/iem_kkt_border_device.h) forms the same ones.
struct KktSumManyArgs { const double *in; double *out; long long rows, w, rows_per_wg, in_ld, out_ld, wgs; };
extern "C" __global__ __launch_bounds__(256) void kkt_colsum_m(const KktSumManyArgs A) {
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

#endif  // IEM_KKT_MANY_DEVICE_H
