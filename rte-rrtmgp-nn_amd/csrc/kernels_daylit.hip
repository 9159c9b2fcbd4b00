// kernels_daylit.hip -- device-side column compaction for the shortwave chain: find the daylit columns of a block,
// gather their rows into dense arrays, and scatter the dense fluxes back with zeros at night.
//
// The RFMIP driver solves every column, the night ones with mu0 = 1 (rrtmgp_rfmip_sw.F90:285-287 usecol, :433 the
// merge), and zeroes their fluxes afterwards (:456-463).  A host model compacts the block to its daylit columns
// instead; these three kernels do that without the host ever seeing the count: nday is one device word, which the
// active-count twins of the SW network (kernels_nn32.hip) and SW solver (kernels_sw_ck.hip) read, so a hipGraph
// captured once follows the sun from replay to replay.
#include "internal.hpp"

namespace rrtmgpnn {

namespace {

// kind 0: daylit iff v < bound (the driver's form on sza); kind 1: daylit iff v > bound (callers that hold mu0).  A NaN
// compares false either way: night
__device__ __forceinline__ bool daylit(float v, int kind, float bound) { return kind == 0 ? v < bound : v > bound; }

constexpr int kPlanThreads = 1024, kPlanWaves = kPlanThreads / 64, kPlanItems = 4;
static_assert(kPlanWaves * kPlanItems == 64, "one lane of wave 0 scans one (item, wave) total");

}  // namespace

// One block.  idx: the daylit columns in increasing order, then the night columns in increasing order; slot[i]: the
// dense position of daylit column i, -1 at night; *nday_out: the count.  A first pass counts (the night columns' places
// start at nday); the second walks chunks of kPlanItems x kPlanThreads columns in order: a ballot and a popcount give a
// lane its rank in its wave, wave 0 scans the chunk's (item, wave) totals in LDS, and a running base carries the chunks
// before.  The places depend on the values alone, never on scheduling.
__global__ void __launch_bounds__(kPlanThreads)
    daylit_plan_kernel(int ncol, const float *__restrict__ v, int kind, float bound, int *__restrict__ idx,
                       int *__restrict__ slot, int *__restrict__ nday_out)
{
  __shared__ int wt[kPlanItems * kPlanWaves];
  __shared__ int total;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int cnt = 0;
  for (int i = tid; i < ncol; i += kPlanThreads) cnt += daylit(v[i], kind, bound) ? 1 : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o);
  if (lane == 0) wt[wave] = cnt;
  __syncthreads();
  if (tid == 0) {
    int s = 0;
    for (int w = 0; w < kPlanWaves; w++) s += wt[w];
    total = s;
  }
  __syncthreads();
  const int nday = total;
  __syncthreads();
  const unsigned long long below = (1ull << lane) - 1ull;
  int run = 0;  // daylit columns of the chunks before this one
  for (int base = 0; base < ncol; base += kPlanItems * kPlanThreads) {
    bool in[kPlanItems], day[kPlanItems];
    int rank[kPlanItems];
#pragma unroll
    for (int k = 0; k < kPlanItems; k++) {
      // (base + k * kPlanThreads + tid can pass 2^31 only past ncol: compared before it is formed)
      in[k] = tid < ncol - base - k * kPlanThreads;
      day[k] = in[k] && daylit(v[in[k] ? base + k * kPlanThreads + tid : 0], kind, bound);
      const unsigned long long b = __ballot(day[k]);
      rank[k] = __popcll(b & below);
      if (lane == 0) wt[k * kPlanWaves + wave] = __popcll(b);
    }
    __syncthreads();
    if (wave == 0) {
      const int x = wt[lane];
      int s = x;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(s, o);
        if (lane >= o) s += u;
      }
      wt[lane] = s - x;
      if (lane == 63) total = s;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kPlanItems; k++) {
      if (in[k]) {
        const int i = base + k * kPlanThreads + tid;
        const int p = run + wt[k * kPlanWaves + wave] + rank[k];  // daylit columns before i
        if (day[k]) {
          idx[p] = i;
          slot[i] = p;
        } else {
          idx[nday + (i - p)] = i;
          slot[i] = -1;
        }
      }
    }
    run += total;
    __syncthreads();
  }
  if (tid == 0) *nday_out = nday;
}

namespace {
constexpr int kColThreads = 256, kColsPerBlock = 64;
}

// Block (x, y): columns [64 x, 64 x + 64) of array y of the table.  Row idx[j] of src to row j of dst for j < *nday;
// blocks past the count exit.  Element by element: rows of any length at any 4-byte alignment
__global__ void __launch_bounds__(kColThreads)
    gather_columns_kernel(int ncol, ColumnTable t, const int *__restrict__ idx, const int *__restrict__ nday_p)
{
  __shared__ int from[kColsPerBlock];
  const int nday = min(*nday_p, ncol);
  const int j0 = blockIdx.x * kColsPerBlock;
  if (j0 >= nday) return;
  const int nj = min(kColsPerBlock, nday - j0);
  if ((int)threadIdx.x < nj) from[threadIdx.x] = idx[j0 + threadIdx.x];
  __syncthreads();
  const int a = blockIdx.y, r = t.row[a];
  const float *__restrict__ src = t.src[a];
  float *__restrict__ dst = t.dst[a];
  for (int e = threadIdx.x; e < nj * r; e += kColThreads) {
    const int jj = e / r, k = e - jj * r;
    dst[(size_t)(j0 + jj) * r + k] = src[(size_t)from[jj] * r + k];
  }
}

// Long rows (an aerosol's band array: (nbnd, nlay) floats per column), where 64 columns per block would leave a block
// hundreds of dependent steps: block (j, y) copies row idx[j] of array y to row j with its lanes side by side; blocks at
// or past the count exit.  Chosen for a table whose rows are all at least kLongRow floats (launch_gather_columns)
namespace {
constexpr int kLongRow = 256;
}
__global__ void __launch_bounds__(kColThreads)
    gather_rows_kernel(int ncol, ColumnTable t, const int *__restrict__ idx, const int *__restrict__ nday_p)
{
  const int j = blockIdx.x;
  if (j >= min(*nday_p, ncol)) return;
  const int a = blockIdx.y, r = t.row[a];
  const float *__restrict__ src = t.src[a] + (size_t)idx[j] * r;
  float *__restrict__ dst = t.dst[a] + (size_t)j * r;
  for (int k = threadIdx.x; k < r; k += kColThreads) dst[k] = src[k];
}

// Block (x, y): columns [64 x, 64 x + 64) of array y.  Column i of out from dense row slot[i], zeros where slot[i] < 0:
// the driver's zeroing of the unused columns, here also of flux_dir
__global__ void __launch_bounds__(kColThreads)
    scatter_columns_kernel(int ncol, ColumnTable t, const int *__restrict__ slot)
{
  __shared__ int from[kColsPerBlock];
  const int i0 = blockIdx.x * kColsPerBlock;
  const int ni = min(kColsPerBlock, ncol - i0);
  if ((int)threadIdx.x < ni) from[threadIdx.x] = slot[i0 + threadIdx.x];
  __syncthreads();
  const int a = blockIdx.y, r = t.row[a];
  const float *__restrict__ src = t.src[a];
  float *__restrict__ dst = t.dst[a];
  for (int e = threadIdx.x; e < ni * r; e += kColThreads) {
    const int ii = e / r, k = e - ii * r;
    const int s = from[ii];
    dst[(size_t)(i0 + ii) * r + k] = s >= 0 ? src[(size_t)s * r + k] : 0.0f;
  }
}

int launch_daylit_plan(rrtmgpnn_context *ctx, int ncol, const float *v, int kind, float bound, int *idx, int *slot,
                       int *nday)
{
  hipLaunchKernelGGL(daylit_plan_kernel, dim3(1), dim3(kPlanThreads), 0, ctx->stream, ncol, v, kind, bound, idx, slot,
                     nday);
  RRTMGPNN_LAUNCH_CHECK("daylit_plan_kernel");
  return RRTMGPNN_OK;
}

int launch_gather_columns(rrtmgpnn_context *ctx, int ncol, const ColumnTable &t, const int *idx, const int *nday)
{
  if (ncol == 0 || t.n == 0) return RRTMGPNN_OK;
  bool long_rows = true;
  for (int a = 0; a < t.n; a++) long_rows = long_rows && t.row[a] >= kLongRow;
  if (long_rows) {
    hipLaunchKernelGGL(gather_rows_kernel, dim3(ncol, t.n), dim3(kColThreads), 0, ctx->stream, ncol, t, idx, nday);
    RRTMGPNN_LAUNCH_CHECK("gather_rows_kernel");
    return RRTMGPNN_OK;
  }
  const dim3 grid((ncol + kColsPerBlock - 1) / kColsPerBlock, t.n);
  hipLaunchKernelGGL(gather_columns_kernel, grid, dim3(kColThreads), 0, ctx->stream, ncol, t, idx, nday);
  RRTMGPNN_LAUNCH_CHECK("gather_columns_kernel");
  return RRTMGPNN_OK;
}

int launch_scatter_columns(rrtmgpnn_context *ctx, int ncol, const ColumnTable &t, const int *slot)
{
  if (ncol == 0 || t.n == 0) return RRTMGPNN_OK;
  const dim3 grid((ncol + kColsPerBlock - 1) / kColsPerBlock, t.n);
  hipLaunchKernelGGL(scatter_columns_kernel, grid, dim3(kColThreads), 0, ctx->stream, ncol, t, slot);
  RRTMGPNN_LAUNCH_CHECK("scatter_columns_kernel");
  return RRTMGPNN_OK;
}

}  // namespace rrtmgpnn
