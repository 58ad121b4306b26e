// artn_rdm_kernel.h -- reduced density matrices of an amplitude array on gfx950: rho[i][j] = sum_r a[i, r] conj(a[j, r]), the Gram
// matrix of the D x (n / D) matrix whose rows are the kept index, read in place from the memory order of a dense (permuted) tensor.
// The Born contract, extended: every product is formed in float64 (complex64 values are converted first, so their products are
// exact), accumulation is float64 on v_mfma_f64_16x16x4_f64, there are no floating-point atomics, and the summation order depends
// on the plan alone: results are bit-identical from run to run.
//
//   artn_k_rdm_stream<T, TRB>   power-of-two extents: lower-triangle tiles x S ranges of the dropped index, one partial tile each
//   artn_k_rdm_finish           adds the partials of an element in ascending order, mirrors, zeroes the diagonal's imaginary part
//   artn_k_rdm_generic<T>       any extents: one workgroup per element of the lower triangle, fixed tree
//
// Streaming form, in bits of the flat memory index.  "Row" bits are the kept bits plus, while there are fewer than four of them,
// the HIGHEST dropped bits ("group" bits: the 16-row MFMA tile is then filled with 16 / D independent r-groups, and the finish
// kernel adds the D x D diagonal blocks of the 16 x 16 Gram matrix -- the off-diagonal blocks are computed and not used).  The
// packed row index has the row bits in ascending memory order; its low TRB bits (4, 5 or 6) index the 2^TRB rows of a tile, the
// others number the tiles.  A PANEL is the 2^10 elements spanned by a tile's TRB row bits and the c = 10 - TRB lowest dropped
// bits: every memory bit below the (c+1)-th dropped bit lies inside it, so a panel is made of contiguous runs of at least
// 2^c elements wherever the kept bits lie, read 16 bytes per lane in ascending address order.
//
// LDS image of a panel: float64, index (2 * col + plane) * RP + row (plane 0 re, 1 im; converted at the store).  One
// v_mfma_f64_16x16x4_f64 (lane roles: artn_gemm128_kernel.h:16) takes kk = lane >> 4 = 2 * cc + p: column 2s + cc, plane p, i.e.
// LDS line 4s + kk, and 16 consecutive rows lane & 15: lane group kk reads 128 contiguous bytes, and with RP = 16 (mod 32)
// doubles the two groups of a 32-lane half of ds_read_b64 fall on disjoint halves of the 64 banks: conflict-free.
//   rho_re block (bi, bj) += A(rows bi, line 4s + kk)     x  B(rows bj, line 4s + kk)              = Ar Ar^T + Ai Ai^T
//   rho_im block (bi, bj) += A(rows bi, line 4s + (kk^1)) x  (p ? -1 : 1) B(rows bj, line 4s + kk) = Ai Ar^T - Ar Ai^T
// Waves of a workgroup (4) split the blocks of the tile (RS ways) and the columns of the panel (KS ways):
//   TRB 4: 1 block,  KS 4                 TRB 5: blocks (0,0) (1,0) (1,1), KS 4
//   TRB 6, diagonal tile: the 10 lower blocks in two lists of 5, KS 2     TRB 6, off-diagonal tile: block row = wave, KS 1
// A wave adds its columns in ascending order, panel after panel in ascending order of the dropped index; at the end the KS
// column shares of a block are added in ascending order through LDS and the tile goes to the workspace.
#ifndef ARTN_RDM_KERNEL_H
#define ARTN_RDM_KERNEL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#define ARTN_RDM_THREADS 256
#define ARTN_RDM_PANEL_BITS 10   /* elements per panel = 2^10: 16 KiB of float64 planes                                   */
#define ARTN_RDM_MIN_BITS 12     /* streaming form: at least 2^12 elements                                                */
#define ARTN_RDM_MAX_DIM_BITS 10 /* D <= 1024                                                                             */
#define ARTN_RDM_TARGET_WGS 512  /* tiles * S reaches this where the dropped index allows: two workgroups on each of 256 CUs */
#define ARTN_RDM_MAX_DIMS 96

typedef double rdm_f64x4 __attribute__((ext_vector_type(4)));

__host__ __device__ inline uint64_t rdm_pdep(uint64_t v, uint64_t mask) { // bit x of v -> the x-th set bit of mask
  uint64_t r = 0;
  for (uint64_t bb = 1; mask; bb <<= 1) {
    const uint64_t low = mask & (~mask + 1);
    if (v & bb) r |= low;
    mask ^= low;
  }
  return r;
}
__host__ __device__ inline uint64_t rdm_pext(uint64_t v, uint64_t mask) {
  uint64_t r = 0;
  for (uint64_t bb = 1; mask; bb <<= 1) {
    const uint64_t low = mask & (~mask + 1);
    if (v & low) r |= bb;
    mask ^= low;
  }
  return r;
}

struct ArtnRdmStream {
  uint64_t row_mask;   // memory bits of a tile's rows (the TRB lowest row bits)
  uint64_t col_mask;   // memory bits of a panel's columns (the c lowest dropped bits)
  uint64_t tile_mask;  // the other row bits: they number the tiles
  uint64_t drop_mask;  // the other dropped bits: they number the panels
  int32_t row_bits, col_bits, tile_bits, drop_bits; // popcounts of the four masks
  int32_t split_bits;  // S = 2^split_bits ranges of the panel index
  int32_t kept_bits;   // D = 2^kept_bits
  int32_t group_bits;  // 16 / D r-groups fill the tile (0 when D >= 16)
  uint8_t row_pos[ARTN_RDM_MAX_DIM_BITS]; // bit x of the output row index -> bit of the packed row index
  uint8_t grp_pos[4];                     // bit y of the group number     -> bit of the packed row index
};

template <int TRB, bool OFF> struct RdmShape {
  static constexpr int TR = 1 << TRB, CB = ARTN_RDM_PANEL_BITS - TRB, COLS = 1 << CB;
  static constexpr int RP = TRB == 4 ? 16 : TR + 16;  // doubles between LDS lines: 16 (mod 32)
  static constexpr int PANEL = 2 * COLS * RP;         // doubles of one panel image
  static constexpr int NB = TRB == 4 ? 1 : TRB == 5 ? 3 : OFF ? 4 : 5;
  static constexpr int KS = TRB == 6 ? (OFF ? 1 : 2) : 4;
  static constexpr int RS = 4 / KS;
};
// doubles of LDS a workgroup needs: the panel image(s), or the column shares of the final reduction
template <int TRB> struct RdmLds { static constexpr int N = TRB == 4 ? 2048 : TRB == 5 ? 4608 : 5120; };

// block b of the list of row-split rs: block row bi (rows of the A side), block column bj
template <int TRB, bool OFF> __device__ __forceinline__ void rdm_block(int rs, int b, int &bi, int &bj) {
  if constexpr (TRB == 4) {
    bi = 0, bj = 0;
  } else if constexpr (TRB == 5) {
    bi = b > 0, bj = b > 1;
  } else if constexpr (OFF) {
    bi = rs, bj = b;
  } else {
    constexpr int I0[5] = {0, 1, 1, 2, 2}, J0[5] = {0, 0, 1, 0, 1}, I1[5] = {2, 3, 3, 3, 3}, J1[5] = {2, 0, 1, 2, 3};
    bi = rs ? I1[b] : I0[b], bj = rs ? J1[b] : J0[b];
  }
}

template <typename T> struct RdmVec;
template <> struct RdmVec<float2> { typedef float4 type; };
template <> struct RdmVec<double2> { typedef double2 type; };

// One tile (ti, tj) over the panels [q0, q0 + nq) of the dropped index; the partial tile goes to out[(row * TR + col) * 2 + {re, im}].
template <typename T, int TRB, bool OFF>
__device__ __forceinline__ void rdm_tile(const T *__restrict__ a, const ArtnRdmStream &p, double *lds, int ti, int tj, long q0, long nq,
                                         double *__restrict__ out) {
  typedef RdmShape<TRB, OFF> S;
  typedef typename RdmVec<T>::type V;
  constexpr int TR = S::TR, RP = S::RP, NB = S::NB, KS = S::KS, RS = S::RS, KC = S::COLS / KS;
  constexpr int EPL = sizeof(T) == 8 ? 2 : 1, NL = (1 << ARTN_RDM_PANEL_BITS) / (ARTN_RDM_THREADS * EPL);
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 15, g = lane >> 4, ks = wave % KS, rs = wave / KS;
  double *X = lds, *Y = OFF ? lds + S::PANEL : lds;

  // copy roles: panel element e = EPL * (tid + 256 u), ascending in memory
  long goff[NL];
  int lidx[NL];
#pragma unroll
  for (int u = 0; u < NL; ++u) {
    const uint64_t off = rdm_pdep((uint64_t)(EPL * (tid + ARTN_RDM_THREADS * u)), p.row_mask | p.col_mask);
    goff[u] = (long)off;
    lidx[u] = (int)rdm_pext(off, p.col_mask) * 2 * RP + (int)rdm_pext(off, p.row_mask);
  }
  const int d1 = (p.row_mask & 1) ? 1 : 2 * RP; // LDS step of memory bit 0 (the second complex64 element of a 16-byte load)
  const long base_a = (long)rdm_pdep((uint64_t)ti, p.tile_mask), base_b = (long)rdm_pdep((uint64_t)tj, p.tile_mask);
  uint64_t dq = rdm_pdep((uint64_t)q0, p.drop_mask);

  V va[NL], vb[OFF ? NL : 1];
  auto issue = [&](uint64_t at) {
#pragma unroll
    for (int u = 0; u < NL; ++u) va[u] = *reinterpret_cast<const V *>(a + base_a + (long)at + goff[u]);
    if constexpr (OFF) {
#pragma unroll
      for (int u = 0; u < NL; ++u) vb[u] = *reinterpret_cast<const V *>(a + base_b + (long)at + goff[u]);
    }
  };
  auto put = [&](double *img, const V &v, int at) {
    if constexpr (EPL == 2) {
      img[at] = (double)v.x, img[at + RP] = (double)v.y, img[at + d1] = (double)v.z, img[at + d1 + RP] = (double)v.w;
    } else {
      img[at] = v.x, img[at + RP] = v.y;
    }
  };

  rdm_f64x4 re[NB], im[NB];
  int bi[NB], bj[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    re[b] = rdm_f64x4{0.0, 0.0, 0.0, 0.0}, im[b] = rdm_f64x4{0.0, 0.0, 0.0, 0.0};
    rdm_block<TRB, OFF>(rs, b, bi[b], bj[b]);
  }

  issue(dq);
  for (long q = 0; q < nq; ++q) {
    __syncthreads(); // (the previous panel's image has been consumed)
#pragma unroll
    for (int u = 0; u < NL; ++u) {
      put(X, va[u], lidx[u]);
      if constexpr (OFF) put(Y, vb[u], lidx[u]);
    }
    __syncthreads();
    if (q + 1 < nq) {
      dq = ((dq | ~p.drop_mask) + 1) & p.drop_mask; // the next value of the panel bits, ascending
      issue(dq);
    }
#pragma unroll
    for (int s = 0; s < KC / 2; ++s) {
      const int line = 2 * (ks * KC + 2 * s);
      const double *xp = X + (line + g) * RP + j, *xq = X + (line + (g ^ 1)) * RP + j, *yp = Y + (line + g) * RP + j;
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const double a_re = xp[bi[b] * 16], a_im = xq[bi[b] * 16], b_re = yp[bj[b] * 16];
        const double b_im = (g & 1) ? -b_re : b_re;
        re[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(a_re, b_re, re[b], 0, 0, 0);
        im[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(a_im, b_im, im[b], 0, 0, 0);
      }
    }
  }

  // the KS column shares of a block, added in ascending order
  if constexpr (KS > 1) {
    __syncthreads();
    if (ks > 0) {
#pragma unroll
      for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          double *slot = lds + ((((ks - 1) * RS + rs) * NB + b) * 8 + 2 * r) * 64 + lane;
          slot[0] = re[b][r], slot[64] = im[b][r];
        }
    }
    __syncthreads();
    if (ks == 0) {
#pragma unroll
      for (int k2 = 1; k2 < KS; ++k2)
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const double *slot = lds + ((((k2 - 1) * RS + rs) * NB + b) * 8 + 2 * r) * 64 + lane;
            re[b][r] += slot[0], im[b][r] += slot[64];
          }
    }
  }
  if (ks == 0) {
    // accumulator register r of lane (j, g): row g + 4r of the block (A side), column j (B side)
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        *reinterpret_cast<double2 *>(out + ((long)(bi[b] * 16 + g + 4 * r) * TR + bj[b] * 16 + j) * 2) = make_double2(re[b][r], im[b][r]);
  }
}

// workgroup = (lower-triangle tile, range s of S): ws[((tile * S + s) * TR * TR + row * TR + col) * 2 + {re, im}]
template <typename T, int TRB>
__global__ __launch_bounds__(ARTN_RDM_THREADS, 2) void artn_k_rdm_stream(const T *__restrict__ a, ArtnRdmStream p, double *__restrict__ ws) {
  __shared__ __attribute__((aligned(16))) double lds[RdmLds<TRB>::N];
  const int tile = (int)(blockIdx.x >> p.split_bits);
  const long s = (long)(blockIdx.x & ((1u << p.split_bits) - 1));
  const long nq = (long)1 << (p.drop_bits - p.split_bits);
  double *out = ws + (long)blockIdx.x * (2L << (2 * TRB));
  if constexpr (TRB == 6) {
    int ti = 0;
    while ((ti + 1) * (ti + 2) / 2 <= tile) ++ti;
    const int tj = tile - ti * (ti + 1) / 2;
    if (ti == tj) rdm_tile<T, 6, false>(a, p, lds, ti, tj, s * nq, nq, out);
    else rdm_tile<T, 6, true>(a, p, lds, ti, tj, s * nq, nq, out);
  } else {
    rdm_tile<T, TRB, false>(a, p, lds, 0, 0, s * nq, nq, out);
  }
}

// One thread per element (oi, oj) of the D x D output.  Its packed rows (pi, pj) are ordered so that pi >= pj (the computed
// triangle); the value is the sum over the groups, ascending, of the sums over the S partials, ascending; the upper triangle is
// the conjugate of the lower one and the diagonal's imaginary part is 0.
__global__ __launch_bounds__(ARTN_RDM_THREADS) void artn_k_rdm_finish(const double *__restrict__ ws, ArtnRdmStream p,
                                                                      double *__restrict__ out) {
  const long o = (long)blockIdx.x * ARTN_RDM_THREADS + threadIdx.x;
  const int k = p.kept_bits;
  if (o >= ((long)1 << (2 * k))) return;
  const unsigned oi = (unsigned)(o >> k), oj = (unsigned)(o & (((long)1 << k) - 1));
  unsigned pi = 0, pj = 0;
  for (int x = 0; x < k; ++x) pi |= ((oi >> x) & 1u) << p.row_pos[x], pj |= ((oj >> x) & 1u) << p.row_pos[x];
  const bool swap = pi < pj, diag = pi == pj;
  if (swap) {
    const unsigned t = pi;
    pi = pj, pj = t;
  }
  const unsigned tr_mask = (1u << p.row_bits) - 1;
  const long S = (long)1 << p.split_bits, tile_doubles = 2L << (2 * p.row_bits);
  double re = 0.0, im = 0.0;
  for (unsigned gg = 0; gg < (1u << p.group_bits); ++gg) {
    unsigned gofs = 0;
    for (int y = 0; y < p.group_bits; ++y) gofs |= ((gg >> y) & 1u) << p.grp_pos[y];
    const unsigned ri = pi | gofs, rj = pj | gofs;
    const long ti = ri >> p.row_bits, tj = rj >> p.row_bits;
    const double *src = ws + (ti * (ti + 1) / 2 + tj) * S * tile_doubles + (((long)(ri & tr_mask) << p.row_bits) + (rj & tr_mask)) * 2;
#pragma unroll 8
    for (long s = 0; s < S; ++s) {
      const double2 v = *reinterpret_cast<const double2 *>(src + s * tile_doubles);
      re += v.x, im += v.y;
    }
  }
  *reinterpret_cast<double2 *>(out + o * 2) = make_double2(re, diag ? 0.0 : swap ? -im : im);
}

// Any extents.  dims [0, n_keep) are the kept ones in output order (last fastest), the others are summed, last fastest.
struct ArtnRdmGeneric {
  int32_t n_keep, n_drop;
  int64_t extent[ARTN_RDM_MAX_DIMS], stride[ARTN_RDM_MAX_DIMS];
};
// Workgroup (i, j), j <= i: thread t adds the terms r = t, t + 256, ... in that order, then a fixed tree over the threads.
template <typename T>
__global__ __launch_bounds__(ARTN_RDM_THREADS) void artn_k_rdm_generic(const T *__restrict__ a, ArtnRdmGeneric p, long D, long n_sum,
                                                                       double *__restrict__ out) {
  __shared__ double red[ARTN_RDM_THREADS][2];
  const long i = blockIdx.x, j = blockIdx.y;
  if (j > i) return;
  long at_i = 0, at_j = 0, ri = i, rj = j;
  for (int d = p.n_keep - 1; d >= 0; --d) {
    at_i += (ri % p.extent[d]) * p.stride[d], ri /= p.extent[d];
    at_j += (rj % p.extent[d]) * p.stride[d], rj /= p.extent[d];
  }
  const int tid = threadIdx.x;
  double re = 0.0, im = 0.0;
  for (long q = tid; q < n_sum; q += ARTN_RDM_THREADS) {
    long r = q, off = 0;
    for (int d = p.n_keep + p.n_drop - 1; d >= p.n_keep; --d) {
      off += (r % p.extent[d]) * p.stride[d];
      r /= p.extent[d];
    }
    const T x = a[at_i + off], y = a[at_j + off];
    const double xr = (double)x.x, xi = (double)x.y, yr = (double)y.x, yi = (double)y.y;
    re += fma(xr, yr, xi * yi);    // Re x conj(y)
    im += fma(xi, yr, -(xr * yi)); // Im x conj(y)
  }
  red[tid][0] = re, red[tid][1] = im;
  __syncthreads();
  for (int s = ARTN_RDM_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid][0] += red[tid + s][0], red[tid][1] += red[tid + s][1];
    __syncthreads();
  }
  if (tid == 0) {
    const double vr = red[0][0], vi = i == j ? 0.0 : red[0][1];
    out[(i * D + j) * 2] = vr, out[(i * D + j) * 2 + 1] = vi;
    if (i != j) out[(j * D + i) * 2] = vr, out[(j * D + i) * 2 + 1] = -vi;
  }
}

#endif // ARTN_RDM_KERNEL_H
