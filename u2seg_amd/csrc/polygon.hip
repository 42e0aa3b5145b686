// Polygon ground truth -> bit planes on the device (gfx950): cocoapi's rleFrPoly restated for the plane layout of maskeval.hip.
// Contract: include/u2seg_hip.h, definition: u2seg_amd/data/polygon.py, design: DESIGN.md section 14.
//
// A polygon's crossings toggle the column-major scan; the mask is the prefix parity of the toggles, which in the plane layout
// (W columns of wpc = ceil(H / 64) words, bit b of word j of column x = pixel (64 j + b, x)) is a parity scan inside every word,
// along the words of a column and along the columns.  Four kernels in stream order:
//   zero    every polygon's toggle plane (the mask's own plane for its first polygon, a scratch plane for the others);
//   toggle  threads over (edge, step) pairs walk the boundary in float64 exactly as the definition does and XOR one bit per
//           crossing into the toggle plane;
//   parity  one work-group per polygon turns the toggle plane into the polygon's mask in place;
//   union   one work-group per mask ORs the further polygons' planes into the mask's and counts its pixels.
// The only atomics are 64-bit integer XORs: the planes do not depend on the order in which they arrive.
#include "common.h"
#include "u2seg_hip.h"

typedef unsigned long long u64;

constexpr int PG_THREADS = 256;
constexpr int PG_MAXJOB = 96;  // jobs of one launch, passed by value
constexpr int PG_SPLIT = 4;    // work-groups that share a polygon's edges (tiles of PG_THREADS edges, round robin)

struct PolyJob { long long tog; int poly, H, W, in_scratch; };  // tog: word offset of the toggle plane in planes or scratch
struct PolyBatch { PolyJob job[PG_MAXJOB]; };
struct UnionJob { long long plane, rest; int H, W, npoly, mask; };  // rest: word offset in scratch of the planes of polygons 1..
struct UnionBatch { UnionJob job[PG_MAXJOB]; };

__device__ __forceinline__ u64* job_plane(const PolyJob& jb, u64* planes, u64* scratch) {
  return (jb.in_scratch ? scratch : planes) + jb.tog;
}
__device__ __forceinline__ int floor_div5(int a) { return a >= 0 ? a / 5 : -((4 - a) / 5); }

// grid (word blocks, jobs)
__global__ __launch_bounds__(PG_THREADS) void poly_zero_kernel(const PolyBatch batch, u64* __restrict__ planes, u64* __restrict__ scratch) {
  const PolyJob jb = batch.job[blockIdx.y];
  const long long nw = (long long)jb.W * ((jb.H + 63) >> 6);
  u64* tog = job_plane(jb, planes, scratch);
  for (long long i = (long long)blockIdx.x * PG_THREADS + threadIdx.x; i < nw; i += (long long)gridDim.x * PG_THREADS) tog[i] = 0ull;
}

// An edge as the definition walks it: `lo` is the stepping coordinate of the end where it is smaller, `other` the other
// coordinate of that end, t the distance from that end; point d (0 = start vertex) has t = flip ? len - d : d.
struct PolyEdge { double s; int lo, other, len, flags; };  // flags: 1 = x is the stepping coordinate, 2 = flip

__device__ __forceinline__ void edge_point(const PolyEdge& e, int d, int& u, int& v) {
  const int t = (e.flags & 2) ? e.len - d : d;
  const int major = t + e.lo;
  int minor = e.other;  // an edge of one point never uses s (0 / 0)
  if (e.len > 0) {
    const double prod = e.s * (double)t;
    const double sum = (double)e.other + prod;
    minor = (int)(sum + .5);
  }
  u = (e.flags & 1) ? major : minor;
  v = (e.flags & 1) ? minor : major;
}

// grid (PG_SPLIT, jobs).  A tile of PG_THREADS edges: every thread sets up one edge, an inclusive scan of the edges' step
// counts goes to LDS, then the threads share the tile's steps (binary search for a step's edge), so that one long edge among
// many short ones is walked by the whole work-group.  Step d of an edge is the pair of its points d - 1 and d; the last point
// of an edge and the first of the next are the same vertex and never cross.
__global__ __launch_bounds__(PG_THREADS) void poly_toggle_kernel(const PolyBatch batch, const double* __restrict__ xy,
                                                                 const long long* __restrict__ poly_offs, u64* __restrict__ planes,
                                                                 u64* __restrict__ scratch) {
  const PolyJob jb = batch.job[blockIdx.y];
  const int H = jb.H, W = jb.W, wpc = (H + 63) >> 6, tx = (int)threadIdx.x;
  const long long v0 = poly_offs[jb.poly], k = poly_offs[jb.poly + 1] - v0;
  u64* tog = job_plane(jb, planes, scratch);
  __shared__ PolyEdge edges[PG_THREADS];
  __shared__ long long scan[2][PG_THREADS];
  for (long long e0 = (long long)blockIdx.x * PG_THREADS; e0 < k; e0 += (long long)gridDim.x * PG_THREADS) {
    const long long e = e0 + tx;
    PolyEdge ed = {0.0, 0, 0, 0, 0};
    if (e < k) {
      const long long a = v0 + e, b = v0 + (e + 1 < k ? e + 1 : 0);
      int xs = (int)(5.0 * xy[2 * a] + .5), ys = (int)(5.0 * xy[2 * a + 1] + .5);
      int xe = (int)(5.0 * xy[2 * b] + .5), ye = (int)(5.0 * xy[2 * b + 1] + .5);
      const int dx = abs(xe - xs), dy = abs(ys - ye);
      const bool xmajor = dx >= dy, flip = (xmajor && xs > xe) || (!xmajor && ys > ye);
      if (flip) { int t = xs; xs = xe; xe = t; t = ys; ys = ye; ye = t; }
      ed.len = xmajor ? dx : dy;
      ed.lo = xmajor ? xs : ys;
      ed.other = xmajor ? ys : xs;
      ed.flags = (xmajor ? 1 : 0) | (flip ? 2 : 0);
      if (ed.len > 0) ed.s = xmajor ? (double)(ye - ys) / (double)dx : (double)(xe - xs) / (double)dy;
    }
    edges[tx] = ed;
    int cur = 0;
    scan[0][tx] = ed.len;
    __syncthreads();
    for (int o = 1; o < PG_THREADS; o <<= 1) {
      scan[cur ^ 1][tx] = scan[cur][tx] + (tx >= o ? scan[cur][tx - o] : 0);
      cur ^= 1;
      __syncthreads();
    }
    const long long* cum = scan[cur];
    const long long total = cum[PG_THREADS - 1];
    for (long long p = tx; p < total; p += PG_THREADS) {
      int lo = 0, hi = PG_THREADS - 1;  // first edge whose inclusive count exceeds p
      while (lo < hi) {
        const int m = (lo + hi) >> 1;
        if (cum[m] > p) hi = m; else lo = m + 1;
      }
      const PolyEdge eg = edges[lo];
      const int d = (int)(p - (lo ? cum[lo - 1] : 0)) + 1;
      int u0, w0, u1, w1;
      edge_point(eg, d - 1, u0, w0);
      edge_point(eg, d, u1, w1);
      if (u1 == u0) continue;
      const int up = u1 < u0 ? u1 : u1 - 1;
      const int q = floor_div5(up);
      if (up - 5 * q != 2 || q < 0 || q >= W) continue;  // xd = (up + .5) / 5 - .5 is the integer q
      int x = q, y = min(max(floor_div5(min(w0, w1) + 2), 0), H);
      if (y == H) { ++x; y = 0; }  // position x H + H is the first pixel of the next column; past the last column: nothing
      if (x < W) atomicXor(tog + (long long)x * wpc + (y >> 6), 1ull << (y & 63));
    }
    __syncthreads();
  }
}

// grid (jobs).  Tiles of PG_THREADS columns: a thread takes the parity of its column's toggles, the parities are scanned over
// the tile (ballot inside a wave, LDS across the four waves, `run` across tiles), then the thread forms the prefix parity of
// its column's words with that carry coming in.  The padding bits of a column's last word are cleared.
__global__ __launch_bounds__(PG_THREADS) void poly_parity_kernel(const PolyBatch batch, u64* __restrict__ planes, u64* __restrict__ scratch) {
  const PolyJob jb = batch.job[blockIdx.x];
  const int H = jb.H, W = jb.W, wpc = (H + 63) >> 6, tx = (int)threadIdx.x, lane = tx & 63, wv = tx >> 6;
  u64* tog = job_plane(jb, planes, scratch);
  __shared__ unsigned wave_par[PG_THREADS / 64];
  unsigned run = 0;
  for (long long x0 = 0; x0 < W; x0 += PG_THREADS) {
    const long long x = x0 + tx;
    u64* col = tog + x * wpc;
    unsigned p = 0;
    if (x < W)
      for (int j = 0; j < wpc; ++j) p ^= (unsigned)__popcll(col[j]);
    const u64 votes = __ballot(p & 1u);
    if (lane == 0) wave_par[wv] = (unsigned)__popcll(votes) & 1u;
    __syncthreads();
    unsigned carry = run ^ ((unsigned)__popcll(votes & ((1ull << lane) - 1ull)) & 1u);
    for (int i = 0; i < PG_THREADS / 64; ++i) {
      if (i < wv) carry ^= wave_par[i];
      run ^= wave_par[i];
    }
    if (x < W)
      for (int j = 0; j < wpc; ++j) {
        u64 v = col[j];
        v ^= v << 1; v ^= v << 2; v ^= v << 4; v ^= v << 8; v ^= v << 16; v ^= v << 32;
        if (carry) v = ~v;
        carry = (unsigned)(v >> 63);
        if (j == wpc - 1 && (H & 63)) v &= (1ull << (H & 63)) - 1ull;
        col[j] = v;
      }
    __syncthreads();
  }
}

// grid (jobs): plane of the mask |= planes of its further polygons; area[mask] = set pixels.  A mask without polygons is zeroed.
__global__ __launch_bounds__(PG_THREADS) void poly_union_kernel(const UnionBatch batch, u64* __restrict__ planes,
                                                                const u64* __restrict__ scratch, int* __restrict__ area) {
  const UnionJob jb = batch.job[blockIdx.x];
  const long long nw = (long long)jb.W * ((jb.H + 63) >> 6);
  u64* plane = planes + jb.plane;
  int a = 0;
  for (long long i = threadIdx.x; i < nw; i += PG_THREADS) {
    u64 v = jb.npoly > 0 ? plane[i] : 0ull;
    for (int p = 0; p + 1 < jb.npoly; ++p) v |= scratch[jb.rest + (long long)p * nw + i];
    if (jb.npoly != 1) plane[i] = v;
    a += __popcll(v);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
  __shared__ int red[PG_THREADS / 64];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0 && area) area[jb.mask] = red[0] + red[1] + red[2] + red[3];
}

static long long poly_mask_words(const U2PolyMask& m) { return (long long)m.W * ((m.H + 63) >> 6); }

extern "C" long long u2_mask_polygon_scratch_words(const U2PolyMask* masks, int num_masks) {
  long long need = 0;
  for (int i = 0; masks && i < num_masks; ++i)
    if (masks[i].H > 0 && masks[i].W > 0 && masks[i].num_polys > 1) need += (long long)(masks[i].num_polys - 1) * poly_mask_words(masks[i]);
  return need;
}

extern "C" int u2_mask_planes_from_polygons(const double* xy, const long long* poly_offs, const U2PolyMask* masks, int num_masks,
                                            void* planes, int* area, void* scratch, long long scratch_words, void* stream) {
  if (num_masks <= 0) return 0;
  if (!masks || !planes || ((uintptr_t)planes & 7) || ((uintptr_t)scratch & 7) || ((uintptr_t)xy & 7)) return -1;
  bool any_poly = false;
  for (int i = 0; i < num_masks; ++i) {
    const U2PolyMask& m = masks[i];
    if (m.H < 0 || m.W < 0 || m.plane_offset < 0 || m.first_poly < 0 || m.num_polys < 0) return -1;
    if ((long long)m.H * m.W >= (1LL << 31) || (long long)m.first_poly + m.num_polys >= (1LL << 31)) return -1;
    any_poly = any_poly || (m.H > 0 && m.W > 0 && m.num_polys > 0);
  }
  if (any_poly && (!xy || !poly_offs)) return -1;
  const long long need = u2_mask_polygon_scratch_words(masks, num_masks);
  if (need > 0 && (!scratch || scratch_words < need)) return -1;
  const hipStream_t s = (hipStream_t)stream;

  // polygons: zero, toggle, parity, PG_MAXJOB polygons per launch
  PolyBatch pb;
  int nj = 0;
  long long max_nw = 0, rest = 0;
  auto flush = [&]() -> int {
    if (nj == 0) return 0;
    const unsigned gx = (unsigned)((max_nw + PG_THREADS - 1) / PG_THREADS);
    hipLaunchKernelGGL(poly_zero_kernel, dim3(gx < 32u ? gx : 32u, nj), dim3(PG_THREADS), 0, s, pb, (u64*)planes, (u64*)scratch);
    U2_CHECK_LAUNCH();
    hipLaunchKernelGGL(poly_toggle_kernel, dim3(PG_SPLIT, nj), dim3(PG_THREADS), 0, s, pb, xy, poly_offs, (u64*)planes, (u64*)scratch);
    U2_CHECK_LAUNCH();
    hipLaunchKernelGGL(poly_parity_kernel, dim3(nj), dim3(PG_THREADS), 0, s, pb, (u64*)planes, (u64*)scratch);
    U2_CHECK_LAUNCH();
    nj = 0;
    max_nw = 0;
    return 0;
  };
  for (int i = 0; i < num_masks; ++i) {
    const U2PolyMask& m = masks[i];
    if (m.H == 0 || m.W == 0) continue;
    const long long nw = poly_mask_words(m);
    for (int p = 0; p < m.num_polys; ++p) {
      PolyJob& jb = pb.job[nj++];
      jb.poly = m.first_poly + p;
      jb.H = m.H;
      jb.W = m.W;
      jb.in_scratch = p > 0;
      jb.tog = p > 0 ? rest : m.plane_offset;
      if (p > 0) rest += nw;
      if (nw > max_nw) max_nw = nw;
      if (nj == PG_MAXJOB) {
        const int rc = flush();
        if (rc) return rc;
      }
    }
  }
  const int rc = flush();
  if (rc) return rc;

  // masks: union and area, after every polygon's plane is complete
  UnionBatch ub;
  int nu = 0;
  rest = 0;
  for (int i = 0; i <= num_masks; ++i) {
    if (i < num_masks && masks[i].H > 0 && masks[i].W > 0) {
      const U2PolyMask& m = masks[i];
      UnionJob& jb = ub.job[nu++];
      jb.plane = m.plane_offset;
      jb.rest = rest;
      jb.H = m.H;
      jb.W = m.W;
      jb.npoly = m.num_polys;
      jb.mask = i;
      if (m.num_polys > 1) rest += (long long)(m.num_polys - 1) * poly_mask_words(m);
    }
    if (nu == PG_MAXJOB || (i == num_masks && nu > 0)) {
      hipLaunchKernelGGL(poly_union_kernel, dim3(nu), dim3(PG_THREADS), 0, s, ub, (u64*)planes, (const u64*)scratch, area);
      U2_CHECK_LAUNCH();
      nu = 0;
    }
  }
  return 0;
}
