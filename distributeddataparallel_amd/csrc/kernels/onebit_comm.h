// 1-bit gradient wire with error feedback (onebit_comm.hip). A bucket of n elements is cut into
// blocks of G = `block` consecutive elements (512 | 1024 | 2048); a payload is `segments` segments
// of cb blocks, each segment cb·G/8 sign bytes followed by cb fp32 scales.
#pragma once

#include <torch/extension.h>

#include <string>

namespace xddp {
namespace kernels {

// v = x + err (x flat fp32 / bf16 / fp16, err flat fp32 of the same length, updated in place to
// v - decoded) -> payload (uint8, segments · cb · (block / 8 + 4) bytes with
// cb = ceil(ceil(numel / block) / segments)); blocks past the last real one are zero
void onebit_compress(const at::Tensor& x, at::Tensor err, at::Tensor payload, int64_t block, int64_t segments);
// mode "mean": the segments cover the same blocks, out = mean over segments of the decoded values;
// mode "concat": the segments cover consecutive block ranges, out = the decoded values
void onebit_decode_mean(const at::Tensor& payload, at::Tensor out, int64_t block, int64_t segments,
                        const std::string& mode);
// payload_out (one segment of cb blocks) = compress(mean over the `segments` segments of payload_in
// + err), err [cb · block] fp32 updated in place; the first `numel` elements of the chunk are real
void onebit_reduce_recompress(const at::Tensor& payload_in, at::Tensor err, at::Tensor payload_out, int64_t block,
                              int64_t segments, int64_t numel);

}  // namespace kernels
}  // namespace xddp
