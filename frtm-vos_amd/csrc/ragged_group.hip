// The refiner's three per-frame places and the mask merge for frames that carry DIFFERENT numbers of objects (a StreamPool group of
// streams with unequal object counts, model/stream_pool.py).  The bodies are those of k_tse_inject, k_cab_gate, k_cab_combine and
// k_track_merge, defined once in per_frame.h; the kernels here hand them a lookup that reads a sample's frame from a device table
// (the frame_of_pair table of frtm_target_apply_grouped, so one table serves the scoring and the refiner) and a merge layout that
// reads each frame's first sample from the table's prefix sums.  What is left in this file: those wrappers, the zeroing of the
// packed counts and the entry points with their argument checks.
#include "frtm_common.h"
#include "resample_taps.h"
#include "per_frame.h"
#include "../../include/frtm_hip.h"

__global__ __launch_bounds__(256) void k_tse_inject_indexed(const float* __restrict__ base, const float* __restrict__ bias,
                                                             const float* __restrict__ ws, const float* __restrict__ scores,
                                                             const int* __restrict__ frame_of, int F, int C, int h, int w, int H, int W,
                                                             float* __restrict__ out) {
  tse_inject_body(base, bias, ws, scores, FrameByTable{frame_of, F}, C, h, w, H, W, out);
}

__global__ __launch_bounds__(256) void k_cab_combine_indexed(const float* __restrict__ shallow, const float* __restrict__ gate,
                                                              const float* __restrict__ deeper, const int* __restrict__ entry_of, int entries,
                                                              int C, int hd, int wd, int H, int W, float* __restrict__ out) {
  cab_combine_body(shallow, gate, deeper, FrameByTable{entry_of, entries}, C, hd, wd, H, W, out);
}

__global__ __launch_bounds__(256) void k_cab_gate_indexed(const float* __restrict__ sp, const float* __restrict__ dp, const int* __restrict__ row_of,
                                                           int rows, const float* __restrict__ W1, const float* __restrict__ b1,
                                                           const float* __restrict__ W2, const float* __restrict__ b2, int oc,
                                                           float* __restrict__ gate) {
  cab_gate_body(sp, dp, FrameByTable{row_of, rows}, W1, b1, W2, b2, oc, gate);
}

// counts of every valid frame to zero (16 threads per frame): the packed size is known on the device only.
__global__ __launch_bounds__(256) void k_ragged_zero_counts(const int* __restrict__ first, int frames, int* __restrict__ counts) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int f = i / MERGE_MAX, k = i % MERGE_MAX;
  if (f >= frames) return;
  size_t logit0, plane0;
  int n;
  if (RaggedFrames{first, frames}(f, logit0, plane0, n) && k <= n) counts[plane0 + k] = 0;
}

// No label decoding: K = n_f + 1 planes per frame, packed.
__global__ __launch_bounds__(256) void k_track_merge_ragged(const float* __restrict__ logits, const int* __restrict__ first, int frames, int HW,
                                                            float* __restrict__ masks, int* __restrict__ counts, float thr) {
  track_merge_body(logits, RaggedFrames{first, frames}, HW, masks, nullptr, nullptr, 0, counts, thr);
}

extern "C" {

int frtm_tse_inject_indexed(const float* base, const float* bias, const float* ws, const float* scores, int n, const int* frame_of, int F,
                            int C, int h, int w, int H, int W, float* out, frtm_stream_t stream) {
  FRTM_CHECK_ARG(base && bias && ws && scores && frame_of && out && n > 0 && C > 0 && F > 0, "frtm_tse_inject_indexed: bad argument");
  FRTM_CHECK_ARG(h > 0 && w > 0 && H > 0 && W > 0, "frtm_tse_inject_indexed: map sizes must be positive (scores %d x %d, maps %d x %d)", h, w, H, W);
  FRTM_CHECK_ARG((size_t)H * W < 0x7fffffff && (size_t)h * w < 0x7fffffff, "frtm_tse_inject_indexed: map too large");
  FRTM_CHECK_ARG((size_t)n * INJ_CG <= 65535, "frtm_tse_inject_indexed: at most %d samples per call (got %d)", 65535 / INJ_CG, n);
  FRTM_CHECK_ARG(ceil_div(H, INJ_TH) <= 65535, "frtm_tse_inject_indexed: at most %d rows per map (got %d)", 65535 * INJ_TH, H);
  dim3 g(ceil_div(W, INJ_TW), ceil_div(H, INJ_TH), n * INJ_CG);
  k_tse_inject_indexed<<<g, 256, 0, (hipStream_t)stream>>>(base, bias, ws, scores, frame_of, F, C, h, w, H, W, out);
  FRTM_LAUNCH_CHECK();
  return FRTM_OK;
}

int frtm_cab_gate_indexed(const float* sp, const float* dp, const int* row_of, int rows, const float* W1, const float* b1, const float* W2,
                          const float* b2, int n, int oc, float* gate, frtm_stream_t stream) {
  FRTM_CHECK_ARG(sp && dp && row_of && W1 && b1 && W2 && b2 && gate && n > 0 && oc > 0 && rows > 0, "frtm_cab_gate_indexed: bad argument");
  // 7 oc floats of dynamic LDS; 64 KB is what a launch gets without raising the kernel's limit
  FRTM_CHECK_ARG((size_t)7 * oc * sizeof(float) <= 65536, "frtm_cab_gate_indexed: oc = %d needs %zu bytes of LDS, more than the 65536 of a default launch",
                 oc, (size_t)7 * oc * sizeof(float));
  FRTM_CHECK_ARG(oc % 4 == 0, "frtm_cab_gate_indexed: oc must be a multiple of 4 (got %d)", oc);
  k_cab_gate_indexed<<<n, 256, 7 * oc * sizeof(float), (hipStream_t)stream>>>(sp, dp, row_of, rows, W1, b1, W2, b2, oc, gate);
  FRTM_LAUNCH_CHECK();
  return FRTM_OK;
}

int frtm_cab_combine_indexed(const float* shallow, const float* gate, const float* deeper, const int* entry_of, int entries, int n, int C,
                             int hd, int wd, int H, int W, float* out, frtm_stream_t stream) {
  FRTM_CHECK_ARG(shallow && gate && deeper && entry_of && out && n > 0 && C > 0 && entries > 0, "frtm_cab_combine_indexed: bad argument");
  FRTM_CHECK_ARG(hd > 0 && wd > 0 && H > 0 && W > 0, "frtm_cab_combine_indexed: map sizes must be positive (deeper %d x %d, maps %d x %d)", hd, wd, H, W);
  FRTM_CHECK_ARG((size_t)n * C <= 65535 && (size_t)H * W < 0x7fffffff && (size_t)hd * wd < 0x7fffffff,
                 "frtm_cab_combine_indexed: at most 65535 planes per call");
  dim3 g(ceil_div(H, CAB_RB), n * C);
  k_cab_combine_indexed<<<g, 256, 0, (hipStream_t)stream>>>(shallow, gate, deeper, entry_of, entries, C, hd, wd, H, W, out);
  FRTM_LAUNCH_CHECK();
  return FRTM_OK;
}

int frtm_track_merge_ragged(const float* logits, int frames, const int* first, int HW, float* masks, int* counts, float thr,
                            frtm_stream_t stream) {
  FRTM_CHECK_ARG(logits && first && masks && HW > 0, "frtm_track_merge_ragged: bad argument");
  FRTM_CHECK_ARG(frames > 0 && frames <= 65535, "frtm_track_merge_ragged: needs 1 <= frames <= 65535 (got %d)", frames);
  hipStream_t st = (hipStream_t)stream;
  if (counts) {
    k_ragged_zero_counts<<<ceil_div(frames * MERGE_MAX, 256), 256, 0, st>>>(first, frames, counts);
    FRTM_LAUNCH_CHECK();
  }
  dim3 g(min(ceil_div(HW, 256 * 4), 256), frames);
  k_track_merge_ragged<<<g, 256, 0, st>>>(logits, first, frames, HW, masks, counts, thr);
  FRTM_LAUNCH_CHECK();
  return FRTM_OK;
}

}  // extern "C"
