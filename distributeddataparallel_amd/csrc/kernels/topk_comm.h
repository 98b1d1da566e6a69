// Top-k sparsified gradient wire with error feedback (topk_comm.hip). A bucket of n elements is cut
// into blocks of G = `block` consecutive elements (1024 | 2048 | 4096), each of which keeps its
// k (8 | 16 | 32 | 64) entries of largest magnitude; a payload is `segments` segments of cb blocks,
// each segment cb·k fp32 values followed by cb·k uint16 offsets within the block.
#pragma once

#include <torch/extension.h>

#include <string>

namespace xddp {
namespace kernels {

// v = x + err (x flat fp32 / bf16 / fp16, err flat fp32 of the same length, updated in place: 0
// where v went into the payload, v elsewhere) -> payload (uint8, segments · cb · 6 k bytes with
// cb = ceil(ceil(numel / block) / segments)); blocks past the last real one hold empty slots
void topk_compress(const at::Tensor& x, at::Tensor err, at::Tensor payload, int64_t block, int64_t k,
                   int64_t segments);
// mode "mean": the segments cover the same blocks, out = mean over segments of the decoded values;
// mode "concat": the segments cover consecutive block ranges, out = the decoded values
void topk_decode_mean(const at::Tensor& payload, at::Tensor out, int64_t block, int64_t k, int64_t segments,
                      const std::string& mode);
// payload_out (one segment of cb blocks) = compress(mean over the `segments` segments of payload_in
// + err), err [cb · block] fp32 updated in place; the first `numel` elements of the chunk are real
void topk_reduce_reselect(const at::Tensor& payload_in, at::Tensor err, at::Tensor payload_out, int64_t block,
                          int64_t k, int64_t segments, int64_t numel);

}  // namespace kernels
}  // namespace xddp
