// 8-bit block-quantized gradient wire (q8_comm.hip). A bucket of n elements is cut into blocks of
// G = `block` consecutive elements (128 | 256 | 512 | 1024); a payload is `segments` segments of
// cb blocks, each segment cb·G code bytes followed by cb (lo, scale) fp32 pairs.
#pragma once

#include <torch/extension.h>

#include <string>

namespace xddp {
namespace kernels {

// x flat fp32 / bf16 / fp16 -> payload (uint8, segments · cb · (block + 8) bytes with
// cb = ceil(ceil(numel / block) / segments)); segment r holds the blocks
// [r·cb, (r + 1)·cb), blocks past the last real one are zero
void q8_quantize(const at::Tensor& x, at::Tensor payload, int64_t block, int64_t segments);
// mode "mean": the segments cover the same blocks, out = mean over segments of the decoded values;
// mode "concat": the segments cover consecutive block ranges, out = the decoded values
void q8_dequantize_mean(const at::Tensor& payload, at::Tensor out, int64_t block, int64_t segments,
                        const std::string& mode);
// payload_out (one segment) = quantize(mean over the `segments` segments of payload_in)
void q8_reduce_requant(const at::Tensor& payload_in, at::Tensor payload_out, int64_t block, int64_t segments);

}  // namespace kernels
}  // namespace xddp
