// The optimizer step and the target re-encoding of the reference's training loop on the device (gnn/trainer.py:70,166-169,231).
//
// 1. k_adam: torch.optim.Adam(lr, betas, eps, weight_decay) -- amsgrad off, maximize off, the decay added to the gradient -- for
//    EVERY parameter of a model in one launch.  torch's own step is seven multi_tensor_apply launches on a model of a few dozen
//    small tensors; the work is a few hundred KB, so the launches are the cost.  The table of this step's tensors travels as the
//    kernel's argument (ADAM_CAPACITY tensors, < 4 KB): no device table to keep alive, no copy to order, and the addresses are the
//    ones the caller read for THIS step (gradients are usually fresh allocations).  The grid walks a list of (tensor, chunk) work
//    items, given as the tensors' first chunk numbers; a work-group finds its tensor by bisection over at most 65 uniform words.
//    Per element, in double from the float32 operands, each stored value rounded once:
//        g = grad + wd p;  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g g;  p -= step_size m / (sqrt(v) / bc2_sqrt + eps)
//    with step_size = lr / (1 - b1^t), bc2_sqrt = sqrt(1 - b2^t) of the tensor's own step count t, and the m and v of the last line
//    the values just stored (the update is a function of the state a checkpoint holds).
//    A parameter may be a view at any float offset: the chunks of a tensor start where p is 16-byte aligned, the up to three
//    elements in front of that and behind the last whole float4 are done one by one.  grad, m and v need not share p's alignment;
//    their 16-byte accesses only promise the 4 bytes every float pointer has.
// 2. k_adapt_angle: adapt_bb_orientation_angle (preprocessor/bounding_box.py:536-563) on a collated batch's y, out of place.
#include "common.h"
#include <math.h>

namespace {

constexpr int ADAM_THREADS = 256;
constexpr int ADAM_CHUNK = 2048;       // elements per work item: two float4 per thread
constexpr int ADAM_CAPACITY = 64;      // tensors per launch
constexpr int ADAM_MAX_BLOCKS = 2048;

struct AdamTensor {
  float* p; const float* g; float* m; float* v;
  int64_t n;
  float step_size, bc2_sqrt, wd;
  int32_t head;                        // elements in front of p's first 16-byte boundary (<= 3, <= n)
};

struct AdamLaunch {
  AdamTensor t[ADAM_CAPACITY];
  int32_t first_chunk[ADAM_CAPACITY + 1];   // tensor i owns the work items [first_chunk[i], first_chunk[i + 1]); every tensor has >= 1
  int32_t n_tensors;
  double beta1, beta2, eps;
};
static_assert(sizeof(AdamLaunch) <= 4096, "the table travels as the kernel's argument");

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));   // a 16-byte access at a float's alignment

__device__ __forceinline__ void adam_element(float& p, const float g32, float& m, float& v, const double step_size,
                                             const double bc2_sqrt, const double wd, const double b1, const double b2,
                                             const double eps) {
  const double g = (double)g32 + wd * (double)p;
  m = (float)(b1 * (double)m + (1.0 - b1) * g);
  v = (float)(b2 * (double)v + (1.0 - b2) * (g * g));
  p = (float)((double)p - step_size * ((double)m / (sqrt((double)v) / bc2_sqrt + eps)));
}

__global__ __launch_bounds__(ADAM_THREADS) void k_adam(const AdamLaunch a) {
  const int total = a.first_chunk[a.n_tensors];
  for (int w = blockIdx.x; w < total; w += gridDim.x) {
    int lo = 0, hi = a.n_tensors;                         // first_chunk[lo] <= w < first_chunk[hi]
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (a.first_chunk[mid] <= w) lo = mid; else hi = mid;
    }
    const AdamTensor& t = a.t[lo];
    const int c = w - a.first_chunk[lo];
    const double ss = t.step_size, bs = t.bc2_sqrt, wd = t.wd;
    if (c == 0 && (int)threadIdx.x < t.head) {            // in front of the aligned body
      const int64_t i = threadIdx.x;
      float p = t.p[i], m = t.m[i], v = t.v[i];
      adam_element(p, t.g[i], m, v, ss, bs, wd, a.beta1, a.beta2, a.eps);
      t.p[i] = p; t.m[i] = m; t.v[i] = v;
    }
    const int64_t begin = t.head + (int64_t)c * ADAM_CHUNK;   // <= n: head <= n and the host counts chunks from n - head
    const int64_t left = t.n - begin;
    const int len = left < ADAM_CHUNK ? (int)left : ADAM_CHUNK;
    const int nvec = len >> 2;
    for (int q = threadIdx.x; q < nvec; q += ADAM_THREADS) {
      const int64_t i = begin + 4 * (int64_t)q;
      f32x4 p = *reinterpret_cast<const f32x4*>(t.p + i);
      const f32x4 g = *reinterpret_cast<const f32x4_a4*>(t.g + i);
      f32x4 m = *reinterpret_cast<const f32x4_a4*>(t.m + i);
      f32x4 v = *reinterpret_cast<const f32x4_a4*>(t.v + i);
#pragma unroll
      for (int k = 0; k < 4; k++) {
        float pk = p[k], mk = m[k], vk = v[k];
        adam_element(pk, g[k], mk, vk, ss, bs, wd, a.beta1, a.beta2, a.eps);
        p[k] = pk; m[k] = mk; v[k] = vk;
      }
      *reinterpret_cast<f32x4*>(t.p + i) = p;
      *reinterpret_cast<f32x4_a4*>(t.m + i) = m;
      *reinterpret_cast<f32x4_a4*>(t.v + i) = v;
    }
    const int tail = len & 3;                              // only a tensor's last chunk has one
    if ((int)threadIdx.x >= ADAM_THREADS - tail) {
      const int64_t i = begin + 4 * (int64_t)nvec + (threadIdx.x - (ADAM_THREADS - tail));
      float p = t.p[i], m = t.m[i], v = t.v[i];
      adam_element(p, t.g[i], m, v, ss, bs, wd, a.beta1, a.beta2, a.eps);
      t.p[i] = p; t.m[i] = m; t.v[i] = v;
    }
  }
}

// one thread per row: the row is copied word for word, the angle of a row that carries a box is replaced
__global__ __launch_bounds__(256) void k_adapt_angle(const uint32_t* __restrict__ y, int64_t ldy, uint32_t* __restrict__ out,
                                                     int64_t ldo, int64_t n, int width) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t* src = y + i * ldy;
  uint32_t* dst = out + i * ldo;
  for (int c = 0; c < width; c++) dst[c] = src[c];
  const float first = __uint_as_float(src[1]);
  if (first != first) return;                              // no box: background row
  const double pi = 3.14159265358979323846;
  const double theta = (double)__uint_as_float(src[5]);
  const double shifted = theta > pi / 2 ? theta - pi : theta;
  dst[5] = __float_as_uint((float)sin(shifted));
}

}  // namespace

extern "C" int32_t rgnn_adam_capacity(void) { return ADAM_CAPACITY; }

extern "C" int rgnn_adam_step(int64_t n_tensors, void* const* param, const void* const* grad, void* const* exp_avg,
                              void* const* exp_avg_sq, const int64_t* numel, const int64_t* step, const double* lr,
                              const double* weight_decay, double beta1, double beta2, double eps, int32_t* launches,
                              rgnn_stream_t stream) {
  RGNN_CHECK_ARG(n_tensors >= 0, "bad tensor count");
  RGNN_CHECK_ARG(n_tensors == 0 || (param && grad && exp_avg && exp_avg_sq && numel && step && lr && weight_decay), "null tables");
  for (int64_t i = 0; i < n_tensors; i++) {
    RGNN_CHECK_ARG(numel[i] >= 0 && step[i] >= 1, "bad element or step count");
    RGNN_CHECK_ARG(numel[i] == 0 || (param[i] && grad[i] && exp_avg[i] && exp_avg_sq[i]), "null tensor");
    RGNN_CHECK_ARG(((uintptr_t)param[i] | (uintptr_t)grad[i] | (uintptr_t)exp_avg[i] | (uintptr_t)exp_avg_sq[i]) % 4 == 0,
                   "float pointers must be 4-byte aligned");
    RGNN_CHECK_ARG(numel[i] / ADAM_CHUNK < (1 << 24), "tensor too large for one launch's work list");
  }
  int n_launch = 0;
  AdamLaunch a{};
  a.beta1 = beta1; a.beta2 = beta2; a.eps = eps;
  int64_t i = 0;
  while (i < n_tensors) {
    int k = 0, chunks = 0;
    for (; i < n_tensors && k < ADAM_CAPACITY; i++) {
      if (numel[i] == 0) continue;
      AdamTensor& t = a.t[k];
      t.p = (float*)param[i]; t.g = (const float*)grad[i]; t.m = (float*)exp_avg[i]; t.v = (float*)exp_avg_sq[i];
      t.n = numel[i];
      const int64_t to_boundary = (4 - (int64_t)(((uintptr_t)param[i] / 4) & 3)) & 3;
      t.head = (int32_t)(to_boundary < t.n ? to_boundary : t.n);
      const double bc1 = 1.0 - pow(beta1, (double)step[i]), bc2 = 1.0 - pow(beta2, (double)step[i]);
      t.step_size = (float)(lr[i] / bc1); t.bc2_sqrt = (float)sqrt(bc2); t.wd = (float)weight_decay[i];
      const int64_t body = t.n - t.head;
      a.first_chunk[k] = chunks;
      chunks += body > 0 ? (int)((body + ADAM_CHUNK - 1) / ADAM_CHUNK) : 1;
      k++;
    }
    if (k == 0) break;
    a.first_chunk[k] = chunks;
    a.n_tensors = k;
    const int blocks = chunks < ADAM_MAX_BLOCKS ? chunks : ADAM_MAX_BLOCKS;
    hipLaunchKernelGGL(k_adam, dim3(blocks), dim3(ADAM_THREADS), 0, (hipStream_t)stream, a);
    RGNN_CHECK_LAUNCH();
    n_launch++;
  }
  if (launches) *launches = n_launch;
  return RGNN_OK;
}

extern "C" int rgnn_adapt_orientation_angle(const float* y, int64_t ldy, float* out, int64_t ldo, int64_t n, int32_t width,
                                            rgnn_stream_t stream) {
  RGNN_CHECK_ARG(n >= 0 && width >= 6 && ldy >= width && ldo >= width, "y is [n, 1 + box] with a rotated box (>= 5 columns)");
  if (n == 0) return RGNN_OK;
  RGNN_CHECK_ARG(y && out && y != out, "null pointers or in place");
  hipLaunchKernelGGL(k_adapt_angle, dim3(rgnn_blocks(n, 256)), dim3(256), 0, (hipStream_t)stream, (const uint32_t*)y, ldy,
                     (uint32_t*)out, ldo, n, width);
  RGNN_CHECK_LAUNCH();
  return RGNN_OK;
}
