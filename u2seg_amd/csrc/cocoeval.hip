// COCO AP on the device (gfx950): the two heavy stages of COCOeval - greedy matching of the score-sorted detections of every
// (image, category) cell to its ground truth, and the precision / recall curves of every (category, area range, detection
// budget, IoU threshold) over all images.  Contract: include/u2seg_hip.h, design: DESIGN.md section 15; the definition is
// evaluation/cocoeval.py (_match_image, accumulate), which these kernels reproduce value for value.
//
// Everything but the IoU, rc and pr quotients is integer work; those are single IEEE operations on exact inputs (the build
// has -ffp-contract=off, so a * b - c stays two roundings as in numpy).  No result depends on the order of an addition: the
// only atomics are integer.
#include "common.h"
#include "u2seg_hip.h"

namespace {

constexpr int CE_LDS_IOU = 1024;   // IoU entries of a cell kept in LDS (8 KB per wave: 16+ waves per CU)
constexpr int CE_LDS_GT = 64;      // ground truth of a cell whose taken-flags are one 64-bit register per lane
constexpr int CE_MAX_AREAS = 8;
constexpr int CE_MAX_LANES = 40;   // (area, threshold) pairs: bits 0..39 of a flag word, the rank above them
constexpr int CE_RANK_SHIFT = 40;
constexpr int CE_SCAN = 256;       // detections per scan chunk = threads of an accumulation work-group
constexpr int CE_MAX_REC = 256;    // recall thresholds

typedef unsigned long long u64;

struct Carve {  // the workspace, every part 16-byte aligned
  long long iou, flags, sflags, sscore, gorder, gtign, nvalid, taken, cellnv, path, total;
};
__host__ __device__ inline long long ce_align(long long n) { return (n + 15) & ~15LL; }
inline Carve ce_carve(long long n_dt, long long n_gt, long long iou_entries, long long n_cells, int K, int A, int T) {
  Carve c;
  long long o = 0;
  c.iou = o;    o += ce_align(8 * iou_entries);
  c.flags = o;  o += ce_align(16 * n_dt);
  c.sflags = o; o += ce_align(16 * n_dt);
  c.sscore = o; o += ce_align(8 * n_dt);
  c.gorder = o; o += ce_align(4LL * A * n_gt);
  c.gtign = o;  o += ce_align((long long)A * n_gt);
  c.nvalid = o; o += ce_align(4LL * K * A);
  c.taken = o;  o += ce_align((long long)A * T * n_gt);
  c.cellnv = o; o += ce_align(4LL * A * n_cells);
  c.path = o;   o += ce_align(n_cells);
  c.total = o;
  return c;
}

// ---- matching ------------------------------------------------------------------------------------------------------------------
// one wave per cell.  Phase 1: all lanes fill the cell's IoU table.  Phase 2: lane a < A orders the ground truth for area
// range a (not ignored first, original order kept).  Phase 3: lane a * T + t walks the detections.
template <bool MASK>
__global__ __launch_bounds__(64) void ce_match_kernel(const U2CocoEvalProblem p, unsigned char* __restrict__ ws, const Carve cv,
                                                      int* __restrict__ rec_match, unsigned char* __restrict__ rec_ign) {
  __shared__ double s_iou[CE_LDS_IOU];
  __shared__ unsigned char s_order[CE_MAX_AREAS][CE_LDS_GT];
  __shared__ u64 s_crowd[CE_MAX_AREAS];
  __shared__ int s_nv[CE_MAX_AREAS];
  const long long cell = blockIdx.x;
  const int lane = (int)threadIdx.x, A = p.A, T = p.T, AT = A * T;
  const long long d0 = p.cell_dt_off[cell], g0 = p.cell_gt_off[cell], io = p.cell_iou_off[cell];
  const int D = (int)(p.cell_dt_off[cell + 1] - d0), G = (int)(p.cell_gt_off[cell + 1] - g0);
  const long long E = (long long)D * G;
  const bool lds = E <= CE_LDS_IOU && G <= CE_LDS_GT;
  double* const iou = reinterpret_cast<double*>(ws + cv.iou) + io;
  int* const gorder = reinterpret_cast<int*>(ws + cv.gorder) + (long long)A * g0;
  unsigned char* const gtign = ws + cv.gtign + (long long)A * g0;
  if (lane == 0) ws[cv.path + cell] = lds ? 0 : 1;

  for (long long e = lane; e < E; e += 64) {
    const int d = (int)(e / G), g = (int)(e - (long long)d * G);
    const bool crowd = p.gt_crowd[g0 + g] != 0;
    double v;
    if (MASK) {
      const long long in = p.inter[p.dt_row[d0 + d] + p.gt_col[g0 + g]];
      const long long ad = p.dt_marea[d0 + d], ag = p.gt_marea[g0 + g];
      const long long un = crowd ? ad : ad + ag - in;
      v = un > 0 ? (double)in / (double)un : 0.0;
    } else {
      const double* db = p.dt_box + 4 * (d0 + d);
      const double* gb = p.gt_box + 4 * (g0 + g);
      const double w = fmin(db[0] + db[2], gb[0] + gb[2]) - fmax(db[0], gb[0]);
      const double h = fmin(db[1] + db[3], gb[1] + gb[3]) - fmax(db[1], gb[1]);
      const double in = (w <= 0 || h <= 0) ? 0.0 : w * h;
      const double ad = db[2] * db[3], ag = gb[2] * gb[3];
      const double un = crowd ? ad : ad + ag - in;
      v = in / un;
    }
    iou[e] = v;
    if (lds) s_iou[e] = v;
  }

  if (lane < A) {
    const double lo = p.area_rng[2 * lane], hi = p.area_rng[2 * lane + 1];
    int n = 0;
    u64 cm = 0;
    for (int pass = 0; pass < 2; ++pass) {
      for (int g = 0; g < G; ++g) {
        const double ar = p.gt_area[g0 + g];
        const bool crowd = p.gt_crowd[g0 + g] != 0;
        const bool ign = crowd || ar < lo || ar > hi;
        if (ign == (pass == 1)) {
          gorder[(long long)lane * G + n] = g;
          gtign[(long long)lane * G + n] = (unsigned char)pass;
          if (lds) {
            s_order[lane][n] = (unsigned char)g;
            if (crowd) cm |= 1ULL << n;
          }
          ++n;
        }
      }
      if (pass == 0) {
        s_nv[lane] = n;
        reinterpret_cast<int*>(ws + cv.cellnv)[cell * A + lane] = n;
        if (n) atomicAdd(reinterpret_cast<int*>(ws + cv.nvalid) + (long long)p.cell_cat[cell] * A + lane, n);
      }
    }
    s_crowd[lane] = cm;
  }
  __syncthreads();

  const bool active = lane < AT;
  const int a = active ? lane / T : 0, t = active ? lane - a * T : 0;
  const double lo = p.area_rng[2 * a], hi = p.area_rng[2 * a + 1];
  const double thr = fmin(p.iou_thrs[t], 1 - 1e-10);
  const int nv = s_nv[a];
  const int Gl = active ? G : 0;
  const u64 crowdm = s_crowd[a];
  u64 taken = 0;
  unsigned char* const gtaken = ws + cv.taken + (long long)AT * g0 + (long long)lane * G;
  const int* const order = gorder + (long long)a * G;
  if (!lds)
    for (int g = 0; g < Gl; ++g) gtaken[g] = 0;

  for (int d = 0; d < D; ++d) {
    double best = thr;
    int match = -1;
    if (lds) {
      for (int g = 0; g < Gl; ++g) {
        if (((taken >> g) & 1) && !((crowdm >> g) & 1)) continue;
        if (match >= 0 && match < nv && g >= nv) break;
        const double v = s_iou[d * G + s_order[a][g]];
        if (v >= best) { best = v; match = g; }
      }
      if (match >= 0) taken |= 1ULL << match;
    } else {
      for (int g = 0; g < Gl; ++g) {
        const int col = order[g];
        if (gtaken[g] && !p.gt_crowd[g0 + col]) continue;
        if (match >= 0 && match < nv && g >= nv) break;
        const double v = iou[(long long)d * G + col];
        if (v >= best) { best = v; match = g; }
      }
      if (match >= 0) gtaken[match] = 1;
    }
    const double ar = p.dt_area[d0 + d];
    const bool outside = ar < lo || ar > hi;
    const bool matched = match >= 0;
    const bool ign = active && (matched ? match >= nv : outside);
    const u64 mb = __ballot(matched), ib = __ballot(ign);
    if (lane == 0) {
      u64* f = reinterpret_cast<u64*>(ws + cv.flags) + 2 * (d0 + d);
      f[0] = mb;
      f[1] = ib | ((u64)d << CE_RANK_SHIFT);
    }
    if (rec_match && active) {
      const int col = !matched ? -1 : (lds ? (int)s_order[a][match] : order[match]);
      rec_match[(d0 + d) * AT + lane] = col + 1;
      rec_ign[(d0 + d) * AT + lane] = ign ? 1 : 0;
    }
  }
}

// ---- accumulation ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ce_gather_kernel(const U2CocoEvalProblem p, unsigned char* __restrict__ ws, const Carve cv) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= p.n_dt) return;
  const long long j = p.perm[i];
  const u64* f = reinterpret_cast<const u64*>(ws + cv.flags) + 2 * j;
  u64* sf = reinterpret_cast<u64*>(ws + cv.sflags) + 2 * i;
  sf[0] = f[0];
  sf[1] = f[1];
  reinterpret_cast<double*>(ws + cv.sscore)[i] = p.dt_score[j];
}

struct I3 { int k, tp, fp; };

__device__ __forceinline__ int wave_iscan(int v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int n = __shfl_up(v, o, 64);
    if (lane >= o) v += n;
  }
  return v;
}
__device__ __forceinline__ double wave_maxscan(double v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double n = __shfl_up(v, o, 64);
    if (lane >= o) v = fmax(v, n);
  }
  return v;
}
// inclusive scan over the 256 threads of a work-group; tot = sum over all of them.  red: 12 ints of LDS.
__device__ __forceinline__ I3 block_scan3(I3 v, int* red, I3& tot) {
  const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
  v.k = wave_iscan(v.k, lane);
  v.tp = wave_iscan(v.tp, lane);
  v.fp = wave_iscan(v.fp, lane);
  __syncthreads();
  if (lane == 63) { red[w] = v.k; red[4 + w] = v.tp; red[8 + w] = v.fp; }
  __syncthreads();
  tot.k = tot.tp = tot.fp = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (i < w) { v.k += red[i]; v.tp += red[4 + i]; v.fp += red[8 + i]; }
    tot.k += red[i]; tot.tp += red[4 + i]; tot.fp += red[8 + i];
  }
  return v;
}
__device__ __forceinline__ double block_maxscan(double v, double* red, double& tot) {
  const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
  v = wave_maxscan(v, lane);
  __syncthreads();
  if (lane == 63) red[w] = v;
  __syncthreads();
  tot = red[0];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (i < w) v = fmax(v, red[i]);
    tot = fmax(tot, red[i]);
  }
  return v;
}

// number of recall thresholds <= x (they ascend)
__device__ __forceinline__ int ce_upper(const double* thr, int R, double x) {
  int lo = 0, hi = R;
  while (lo < hi) {
    const int m = (lo + hi) >> 1;
    if (thr[m] <= x) lo = m + 1; else hi = m;
  }
  return lo;
}

// one work-group per (category, area range, budget, threshold).  Pass 1 walks the category's sorted list forwards in chunks of
// CE_SCAN with a carry: inclusive scans of kept / tp / fp; the element at which tp first reaches a recall threshold (and the
// first kept element, for the thresholds its recall already covers) is that threshold's index.  Pass 2 walks backwards: with
// the totals known, tp and fp of an element follow from suffix sums, and the precision envelope is a suffix maximum.
__global__ __launch_bounds__(CE_SCAN) void ce_accumulate_kernel(const U2CocoEvalProblem p, const unsigned char* __restrict__ ws,
                                                                const Carve cv, double* __restrict__ precision,
                                                                double* __restrict__ scores, double* __restrict__ recall) {
  __shared__ double s_thr[CE_MAX_REC], s_prec[CE_MAX_REC], s_score[CE_MAX_REC], s_val[CE_SCAN], s_dred[4];
  __shared__ long long s_idx[CE_MAX_REC];
  __shared__ int s_ired[12];
  const int A = p.A, T = p.T, M = p.M, R = p.R, K = p.K, tid = (int)threadIdx.x;
  int b = (int)blockIdx.x;
  const int t = b % T; b /= T;
  const int m = b % M; b /= M;
  const int a = b % A;
  const int k = b / A;
  const int nv = reinterpret_cast<const int*>(ws + cv.nvalid)[k * A + a];
  if (nv == 0) return;  // the tables are pre-filled with -1
  const int budget = p.max_dets[m], bit = a * T + t;
  const long long L0 = p.cat_dt_off[k], L = p.cat_dt_off[k + 1] - L0;
  const u64* sf = reinterpret_cast<const u64*>(ws + cv.sflags) + 2 * L0;
  const double* ssc = reinterpret_cast<const double*>(ws + cv.sscore) + L0;
  for (int r = tid; r < R; r += CE_SCAN) { s_thr[r] = p.rec_thrs[r]; s_idx[r] = -1; s_prec[r] = 0.0; s_score[r] = 0.0; }
  __syncthreads();

  auto load = [&](long long q, int& ftp, int& ffp) -> int {
    if (q >= L) { ftp = ffp = 0; return 0; }
    const u64 mw = sf[2 * q], iw = sf[2 * q + 1];
    const int keep = (int)(iw >> CE_RANK_SHIFT) < budget ? 1 : 0;
    const int mt = (int)((mw >> bit) & 1), ig = (int)((iw >> bit) & 1);
    ftp = keep & mt & (ig ^ 1);
    ffp = keep & (mt ^ 1) & (ig ^ 1);
    return keep;
  };

  I3 carry = {0, 0, 0};
  for (long long c0 = 0; c0 < L; c0 += CE_SCAN) {
    const long long q = c0 + tid;
    I3 f, tot;
    f.k = load(q, f.tp, f.fp);
    const int keep = f.k, ftp = f.tp;
    I3 s = block_scan3(f, s_ired, tot);
    s.k += carry.k; s.tp += carry.tp;
    if (keep && (s.k == 1 || ftp)) {
      const int hi = ce_upper(s_thr, R, (double)s.tp / (double)nv);
      const int lo = s.k == 1 ? 0 : ce_upper(s_thr, R, (double)(s.tp - ftp) / (double)nv);
      const double sc = ssc[q];
      for (int r = lo; r < hi; ++r) { s_idx[r] = q; s_score[r] = sc; }
    }
    carry.k += tot.k; carry.tp += tot.tp; carry.fp += tot.fp;
  }
  __syncthreads();
  if (tid == 0) recall[(((long long)t * K + k) * A + a) * M + m] = carry.k ? (double)carry.tp / (double)nv : 0.0;

  I3 suf = {0, 0, 0};
  double cmax = -1.0;
  for (long long c0 = (L - 1) / CE_SCAN * CE_SCAN; c0 >= 0 && L > 0; c0 -= CE_SCAN) {
    const long long q = c0 + (CE_SCAN - 1 - tid);  // thread order = reverse list order: a forward scan is a suffix scan
    I3 f, tot;
    f.k = load(q, f.tp, f.fp);
    const int keep = f.k, ftp = f.tp, ffp = f.fp;
    const I3 s = block_scan3(f, s_ired, tot);
    const int tp = carry.tp - (s.tp + suf.tp - ftp), fp = carry.fp - (s.fp + suf.fp - ffp);
    double pr = -1.0;
    if (keep) pr = (tp + fp) > 0 ? (double)tp / (double)(tp + fp) : 0.0;
    double ctot;
    pr = fmax(block_maxscan(pr, s_dred, ctot), cmax);
    s_val[CE_SCAN - 1 - tid] = pr;
    __syncthreads();
    for (int r = tid; r < R; r += CE_SCAN)
      if (s_idx[r] >= c0 && s_idx[r] < c0 + CE_SCAN) s_prec[r] = s_val[s_idx[r] - c0];
    cmax = fmax(cmax, ctot);
    suf.tp += tot.tp; suf.fp += tot.fp;
    __syncthreads();
  }
  for (int r = tid; r < R; r += CE_SCAN) {
    const long long o = ((((long long)t * R + r) * K + k) * A + a) * M + m;
    precision[o] = s_idx[r] >= 0 ? s_prec[r] : 0.0;
    scores[o] = s_score[r];
  }
}

__global__ void ce_fill_kernel(double* __restrict__ x, long long n, double v) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) x[i] = v;
}

bool ce_shapes_ok(const U2CocoEvalProblem* p) {
  return p && p->A >= 1 && p->A <= CE_MAX_AREAS && p->T >= 1 && p->A * p->T <= CE_MAX_LANES && p->M >= 1 && p->R >= 1 &&
         p->R <= CE_MAX_REC && p->K >= 1 && p->n_cells >= 0 && p->n_dt >= 0 && p->n_gt >= 0 && p->n_dt < (1LL << 31) &&
         p->n_gt < (1LL << 31) && p->iou_entries >= 0 && p->max_rank < (1 << 23) &&
         (long long)p->K * p->A * p->M * p->T < (1LL << 31);
}

}  // namespace

extern "C" int u2_cocoeval_lds_iou_entries(void) { return CE_LDS_IOU; }
extern "C" int u2_cocoeval_lds_max_gt(void) { return CE_LDS_GT; }
extern "C" int u2_cocoeval_scan_chunk(void) { return CE_SCAN; }

extern "C" long long u2_cocoeval_workspace_layout(long long n_dt, long long n_gt, long long iou_entries, long long n_cells, int K,
                                                  int A, int T, long long* offsets) {
  if (n_dt < 0 || n_gt < 0 || iou_entries < 0 || n_cells < 0 || K < 0 || A < 0 || T < 0) return -1;
  const Carve c = ce_carve(n_dt, n_gt, iou_entries, n_cells, K, A, T);
  if (offsets) {
    const long long o[10] = {c.iou, c.flags, c.sflags, c.sscore, c.gorder, c.gtign, c.nvalid, c.taken, c.cellnv, c.path};
    for (int i = 0; i < 10; ++i) offsets[i] = o[i];
  }
  return c.total;
}
extern "C" long long u2_cocoeval_workspace_bytes(long long n_dt, long long n_gt, long long iou_entries, long long n_cells, int K,
                                                 int A, int T) {
  return u2_cocoeval_workspace_layout(n_dt, n_gt, iou_entries, n_cells, K, A, T, nullptr);
}

extern "C" int u2_cocoeval_match(const U2CocoEvalProblem* p, void* workspace, long long workspace_bytes, int* rec_match,
                                 unsigned char* rec_ignore, void* stream) {
  if (!ce_shapes_ok(p) || !workspace) return -1;
  if ((rec_match == nullptr) != (rec_ignore == nullptr)) return -1;
  const Carve cv = ce_carve(p->n_dt, p->n_gt, p->iou_entries, p->n_cells, p->K, p->A, p->T);
  if (workspace_bytes < cv.total || ((uintptr_t)workspace & 15)) return -1;
  if (p->n_cells >= (1LL << 31)) return -1;
  if (p->n_cells && (!p->cell_dt_off || !p->cell_gt_off || !p->cell_iou_off || !p->cell_cat || !p->area_rng || !p->iou_thrs)) return -1;
  if (p->n_dt && (!p->dt_area || !p->dt_score || !p->perm)) return -1;
  if (p->n_gt && (!p->gt_area || !p->gt_crowd)) return -1;
  if (p->mask_form) {
    if (p->iou_entries && (!p->inter || !p->dt_row || !p->gt_col || !p->dt_marea || !p->gt_marea)) return -1;
  } else if (p->iou_entries && (!p->dt_box || !p->gt_box)) {
    return -1;
  }
  const hipStream_t s = (hipStream_t)stream;
  unsigned char* ws = (unsigned char*)workspace;
  u2_zero_words(ws + cv.nvalid, (size_t)p->K * p->A, s);
  U2_CHECK_LAUNCH();
  if (p->n_cells == 0) return 0;
  if (p->mask_form)
    hipLaunchKernelGGL(ce_match_kernel<true>, dim3((unsigned)p->n_cells), dim3(64), 0, s, *p, ws, cv, rec_match, rec_ignore);
  else
    hipLaunchKernelGGL(ce_match_kernel<false>, dim3((unsigned)p->n_cells), dim3(64), 0, s, *p, ws, cv, rec_match, rec_ignore);
  U2_CHECK_LAUNCH();
  return 0;
}

extern "C" int u2_cocoeval_accumulate(const U2CocoEvalProblem* p, void* workspace, long long workspace_bytes, double* precision,
                                      double* scores, double* recall, void* stream) {
  if (!ce_shapes_ok(p) || !workspace || !precision || !scores || !recall) return -1;
  const Carve cv = ce_carve(p->n_dt, p->n_gt, p->iou_entries, p->n_cells, p->K, p->A, p->T);
  if (workspace_bytes < cv.total || ((uintptr_t)workspace & 15)) return -1;
  if (!p->cat_dt_off || !p->max_dets || !p->rec_thrs) return -1;
  const hipStream_t s = (hipStream_t)stream;
  unsigned char* ws = (unsigned char*)workspace;
  const long long nr = (long long)p->T * p->K * p->A * p->M, np_ = nr * p->R;
  hipLaunchKernelGGL(ce_fill_kernel, dim3(256), dim3(256), 0, s, precision, np_, -1.0);
  hipLaunchKernelGGL(ce_fill_kernel, dim3(256), dim3(256), 0, s, scores, np_, -1.0);
  hipLaunchKernelGGL(ce_fill_kernel, dim3(64), dim3(256), 0, s, recall, nr, -1.0);
  U2_CHECK_LAUNCH();
  if (p->n_dt) {
    hipLaunchKernelGGL(ce_gather_kernel, dim3((unsigned)((p->n_dt + 255) / 256)), dim3(256), 0, s, *p, ws, cv);
    U2_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(ce_accumulate_kernel, dim3((unsigned)(p->K * p->A * p->M * p->T)), dim3(CE_SCAN), 0, s, *p, ws, cv, precision,
                     scores, recall);
  U2_CHECK_LAUNCH();
  return 0;
}
