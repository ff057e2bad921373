// What the list-attention kernels (attention.hip) and the builders of their block tables (k_blk_tab of
// serial_attention.hip, k_attn_context_lists) agree on.
#pragma once

namespace me {

// The stationary rows of a workgroup: BQ of the forward and dQ kernels, BK of the dK / dV kernel.
constexpr int kAttnBlock = 64;

// The block table of a row list of n rows in n_seg segments: ceil(n / kAttnBlock) + n_seg int32 pairs (segment, first row
// in the segment), one per workgroup of that side's grid: the blocks of the non-empty segments in ascending segment
// order, then unused pairs, which hold segment -1.

}  // namespace me
