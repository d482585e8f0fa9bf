// wbx_record.hip — the recorder tap of Engine::process (engine.cpp:1638-1649) and the recorder thread's copy into the
// take (write_recorded_samples_, engine.cpp:1677-1697) as one kernel: the block the audio thread staged in pinned host
// memory is read once and scattered into every take that records one of its channels, straight into the take's chunks in
// HBM.  Launched on the context's upload stream beside the callback; nothing on the audio thread waits for it.
#include "wbx_ctx.h"

namespace wbx {

namespace {

// One lane per (input channel, frame) of the staged block.  Take k records input channels ch0 .. ch0 + n - 1 (desc[k] =
// ch0 << 2 | n, 0: not this block — the take has no room, or was discarded); frame f of the block is the take's frame
// start + f, which lies in chunk (start + f) / chunk at (start + f) % chunk: a block that straddles chunk boundaries splits
// there.  The samples move as 32-bit words, so every bit pattern (NaN payloads, -0, subnormals) arrives unchanged.
__global__ void __launch_bounds__(256) record_capture_kernel(RecCaptureArgs a) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= a.in_channels * a.frames) return;
  const uint32_t c = i / a.frames, f = i - c * a.frames;
  const uint32_t v = a.stage[(size_t)c * a.frames + f];
  const uint64_t pos = a.start + f;
  const uint64_t chunk = pos / a.chunk_frames;
  const uint32_t off = (uint32_t)(pos - chunk * a.chunk_frames);
  for (uint32_t k = 0; k < a.n_takes; k++) {
    const uint32_t d = a.desc[k];
    const uint32_t ch0 = d >> 2, n = d & 3u;
    if (n == 0u || c < ch0 || c >= ch0 + n) continue;
    uint32_t* row = a.table[(size_t)k * a.table_cap + chunk].ch[c - ch0];
    row[off] = v;
  }
}

}  // namespace

void launch_record_capture(const RecCaptureArgs& a, hipStream_t s) {
  const uint32_t n = a.in_channels * a.frames;
  hipLaunchKernelGGL(record_capture_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, a);
}

}  // namespace wbx
