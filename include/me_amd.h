/*
 * me_amd.h — C ABI of the MI355X (gfx950) sparse-convolution hot path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no torch / pybind types.  Every pointer
 * named *_dev is DEVICE memory owned by the caller (in the PyTorch-ROCm host layer these are
 * tensor.data_ptr() values, so the torch caching allocator plays the role of the reference's
 * c10 allocator, src/allocators.cuh:74-103).  `stream` is a hipStream_t passed as void*; all
 * work is enqueued on it and nothing synchronises the device except the functions documented
 * as "SYNC" (they must return a count to the host, exactly where the reference synchronises).
 *
 * Each entry point cites the reference interface (path:line under the MinkowskiEngine tree) that
 * it replaces.  The reference reaches those through pybind11 (pybind/extern.hpp); INTEGRATION.md
 * shows the binding a maintainer would add.
 *
 * Return value: 0 on success, non-zero on error; me_last_error() describes the last failure of
 * the calling thread (mirrors the reference's ASSERT -> std::runtime_error, src/utils.hpp:141-150).
 */
#ifndef ME_AMD_H
#define ME_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* libme_amd.so is built with -fvisibility=hidden: the entry points declared in this header (and the test hooks of
 * csrc/me_amd_debug.h) are its ONLY exported symbols — no C++ internals, no device stubs. */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define ME_MAX_DIM 7 /* spatial dimensions D; coordinates carry D+1 int32 (batch index first) */

/* region types: src/types.hpp:148-152 (RegionType::HYPER_CUBE / HYPER_CROSS / CUSTOM) */
#define ME_REGION_HYPER_CUBE 0
#define ME_REGION_HYPER_CROSS 1
#define ME_REGION_CUSTOM 2

/* Kernel geometry of one layer; replaces gpu_kernel_region (src/kernel_region.hpp:283-398).
 * Neighbour offsets follow kernel_region.hpp:198-247 (axis 0 fastest; odd sizes centred, even
 * sizes start at 0; multiplied by dilation * tensor_stride).
 * ME_REGION_CUSTOM (the reference declares it and stops at `case CUSTOM: // TODO`; the semantics are this library's):
 * tap k looks up u + offsets_dev[k] * dilation * tensor_stride per axis, so the offsets are in units of the tensor
 * stride, as kernel_size is.  Rows may come in any order and need not hold the origin; kernel_size is ignored and the
 * volume is n_offsets.  The table stays on the device for as long as a launch that got this region may run.  A
 * `me_region r = {}` of a built-in type leaves both trailing fields zero. */
typedef struct me_region {
  int32_t ncol;                    /* D + 1 */
  int32_t region_type;             /* ME_REGION_* */
  int32_t kernel_size[ME_MAX_DIM]; /* per spatial axis */
  int32_t dilation[ME_MAX_DIM];
  int32_t tensor_stride[ME_MAX_DIM]; /* tensor stride of the map that is LOOKED UP (the "in" map) */
  int32_t n_offsets;               /* ME_REGION_CUSTOM: rows K of offsets_dev (ABI 1.13); 0 otherwise */
  const int32_t *offsets_dev;      /* ME_REGION_CUSTOM: int32 [K, D] contiguous, on the device; NULL otherwise */
} me_region;

/* ---- library ------------------------------------------------------------------------------- */
/* 100 * major + 10 * minor.  Changelog:
 *   1.0 (100)  round 1: coordinate maps, kernel maps, tile plans, fp32 / bf16 convolution, pooling
 *   1.1        round 2: tile_bptr_dev grew to 2 * num_tiles + 1 int32 (dispatch order behind the batch ranges) — an
 *              ABI change without a size argument; LDS-bucketed kernel-map build; split fp32 kernels
 *   1.2 (120)  round 3: me_plan_tile_bptr_elems sizes that buffer; me_debug_* hooks left this header
 *              (csrc/me_amd_debug.h: tests / tuning only)
 *   1.3 (130)  round 3: batch-norm statistics in the convolution's epilogue (me_conv_target_bf16_stats,
 *              me_conv_stats_supported_bf16, me_bn_stats_from_tiles)
 *   1.4 (140)  round 4: split-K launches of the bf16 convolution for small coordinate maps
 *              (me_conv_plan_config_bf16_ex, me_conv_splitk_workspace_bytes, me_conv_target_bf16_ex); float64
 *              features (me_conv_target_f64, me_conv_wgrad_f64, me_pool_*_f64, me_global_pool_f64, me_broadcast_f64);
 *              all tile plans of a scene in four launches (me_plan_job, me_plan_jobs_init, me_plan_build_multi)
 *   1.5 (150)  round 5: bf16 convolution on an LDS-staged source halo with register accumulators
 *              (me_conv_halo_config_bf16, me_halo_plan_build, me_conv_halo_bf16); stacked-offset kernel for layers
 *              with at most 8 source channels (me_conv_stem_use_bf16, me_conv_stem_tile_rows, me_conv_stem_bf16)
 *   1.6 (160)  round 6: row-wise launches for kernel-map sides with exactly one pair per target row — K = 1 layers
 *              (the reference's `input.F.mm(kernel)`) and the fine side of kernel_size == stride maps
 *              (me_conv_rowwise_supported_bf16, me_conv_rowwise_bf16); Z-order of a map by the library's own radix sort
 *              (me_coords_zorder)
 *   1.7 (170)  round 7: channelwise (depthwise) convolution, forward and backward (me_cwconv_forward_*,
 *              me_cwconv_backward_workspace_bytes, me_cwconv_backward_*)
 *   1.8 (180)  round 8: tensor fields: quantisation, field -> sparse lookup and trilinear interpolation maps (me_field_*), stable
 *              CSR from COO and the weighted CSR gather-sum (me_csr_*)
 *   1.9 (190)  round 9: instance normalisation: per-instance statistics, apply and backward (me_inorm_workspace_bytes,
 *              me_inorm_stats, me_inorm_apply, me_inorm_backward and their _f64 twins)
 *   1.10 (200) round 10: dense <-> sparse conversion: cell indices, the row grid, the two movers, occupied cells and all
 *              cells of a box (me_dense_*)
 *   1.11 (210) round 11: direct max pooling over an (in_map, out_map) pair list (me_direct_max_pool_*) and the origin-map
 *              row table of a tensor field (me_field_origin_rows_f32)
 *   1.12 (220) round 12: arithmetic between two sparse tensors on different coordinate maps: the row tables of a union
 *              (me_union_tables) and the fused one-write-per-row forward / gather backward (me_union_arith_*)
 *   1.13 (230) round 13: ME_REGION_CUSTOM: me_region grew two trailing fields (n_offsets, offsets_dev); every entry point
 *              that takes a region accepts it, the LDS-bucketed probe declines it (me_kernel_map_probe_lds_bytes: -1)
 *   1.14 (240) round 14: synchronised batch norm on the batch-norm kernels: a rank's (count, mean, M2) record, the merge of
 *              the ranks' records, backward sums without the apply, their sum in rank order and the apply with the global
 *              row count (me_bn_moments_floats, me_bn_local_moments, me_bn_stats_from_moments, me_bn_backward_sums,
 *              me_bn_backward_reduce, me_bn_backward_apply)
 *   1.15 (250)  round 15: group normalisation per (instance, group of channels): statistics, apply and backward
 *              (me_gnorm_workspace_bytes, me_gnorm_stats, me_gnorm_apply, me_gnorm_backward and their _f64 twins)
 *   1.16 (260)  round 16: conditional group normalisation: a per-instance scale / shift folded into the affine map and a
 *              fused SiLU (me_gnorm_cond_workspace_bytes, me_gnorm_cond_apply, me_gnorm_cond_backward and their _f64
 *              twins)
 *   1.17 (270)  round 17: per-instance multi-head attention over the rows of a coordinate map: forward and backward on
 *              the MFMA pipe through per-instance row lists (me_attn_workspace_bytes, me_attn_forward, me_attn_backward
 *              and the _f64 twins me_attn_forward_f64, me_attn_backward_f64)
 *   1.18 (280)  round 18: local attention over a kernel map: every out row attends to the in rows of its kernel region,
 *              with an optional per-head, per-offset bias; gather kernels on the neighbour tables, no atomics
 *              (me_local_attn_workspace_bytes, me_local_attn_forward, me_local_attn_backward and the _f64 twins
 *              me_local_attn_forward_f64, me_local_attn_backward_f64)
 *   1.19 (290)  round 19: serialized patch attention: z-order / Hilbert keys, patch row lists with a block table, and the
 *              attention kernels reading their block from that table instead of walking seg_ptr (me_coords_serial_keys,
 *              me_attn_patch_lists_workspace_bytes, me_attn_patch_lists, me_attn_forward_tab, me_attn_backward_tab and
 *              the _f64 twins me_attn_forward_tab_f64, me_attn_backward_tab_f64)
 *   1.20 (300)  round 20: cross-attention to a dense context: the row lists of a [B, L, C] context in one launch, and a
 *              dK / dV pass split over the queries with a fixed-order reduce for few keys under many queries
 *              (me_attn_context_lists, me_attn_kv_splits, me_attn_split_workspace_bytes, me_attn_backward_split and the
 *              _f64 twin me_attn_backward_split_f64)
 *   1.21 (310)  round 21: shifted-window attention: the window of every row of a coordinate map (boxes of w cells on a grid
 *              anchored at the origin and moved by a shift), and row lists with a block table from any segment id per row
 *              (me_attn_window_ids_workspace_bytes, me_attn_window_ids, me_attn_segment_lists_workspace_bytes,
 *              me_attn_segment_lists)
 *   1.22 (320)  round 22: rotary position embedding from voxel coordinates: the (cos, sin) table of a coordinate map and the
 *              rotation of the channel pairs of strided rows, forward and backward (me_rope_table, me_rope_apply) */
int me_version(void);
const char *me_last_error(void);
/* Load the device code of every translation unit of the library now (needs a GPU; ABI 1.5): HIP loads a unit's code object
 * at the first launch from it, which put 88 ms into the first backward pass of a process.  The hosts call it at the first
 * map insert on a device, under that device's guard (code objects are per device) — not at import. */
int me_preload(void);
/* kernel volume of a region: src/kernel_region.hpp:250-270 (set_volume); n_offsets for ME_REGION_CUSTOM (host only:
 * the table is not read); -1 for an invalid region */
int64_t me_region_volume(const me_region *region);

/* ---- coordinate hash map (replaces CoordinateMapGPU, src/coordinate_map_gpu.cuh:47-223) ------ */

/* Number of 8-byte slots for n keys: power of two >= 2n (<= 50 % load; the reference uses 25-50 %,
 * src/coordinate_map_manager.hpp:139-155). */
int64_t me_hash_capacity(int64_t n);
/* Scratch bytes needed by me_coords_insert_and_map for n rows. */
int64_t me_insert_workspace_bytes(int64_t n);

/* insert + dedup + row maps.  Replaces CoordinateMapGPU::insert<true>
 * (src/coordinate_map_gpu.cu:196-278) but with the CPU path's deterministic semantics
 * (CoordinateMapCPU::insert_and_map, src/coordinate_map_cpu.hpp:353-380): the FIRST occurrence of
 * a coordinate wins and unique rows keep first-occurrence order.
 *   coords_dev      int32 [n, ncol] contiguous (16-byte aligned when ncol == 4)
 *   table_dev       uint64 [capacity]          (out) open-addressing table {hash tag, row}
 *   coords_unique   int32 [n, ncol]            (out) first n_unique rows valid
 *   unique_map_dev  int64 [n]                  (out) first n_unique valid: input row of each unique row
 *   inverse_map_dev int64 [n]                  (out) unique row of each input row
 *   n_unique        host int64                 (out)  — SYNC (one 8-byte D2H copy)
 */
int me_coords_insert_and_map(const int32_t *coords_dev, int64_t n, int32_t ncol, uint64_t *table_dev,
                             int64_t capacity, int32_t *coords_unique_dev, int64_t *unique_map_dev,
                             int64_t *inverse_map_dev, int64_t *n_unique, void *workspace_dev,
                             int64_t workspace_bytes, void *stream);

/* out[i] = floor(c / ts_out) * ts_out on the spatial columns, batch column copied.
 * Replaces stride_copy (src/coordinate_map_gpu.cu:363-397; CPU detail::stride_coordinate,
 * src/coordinate_map.hpp:58-66).  Integer floor division (== the reference's float floor for
 * |c| < 2^24). */
int me_coords_stride(const int32_t *coords_dev, int64_t n, int32_t ncol,
                     const int32_t *out_tensor_stride /* host [ncol-1] */, int32_t *out_coords_dev,
                     void *stream);

/* keys[i] = Z-order (Morton) key of coordinate row i: batch index on top, then the bit-interleaved
 * spatial coordinates in units of the tensor stride.  Sorting target rows by this key gives the tile
 * plan spatially compact tiles (their gathers then hit the L2 instead of HBM).  No reference
 * counterpart (the reference never reorders work); the row order of the maps is NOT changed. */
int me_coords_spatial_keys(const int32_t *coords_dev, int64_t n, int32_t ncol,
                           const int32_t *tensor_stride /* host [ncol-1] */, int64_t *keys_dev, void *stream);
/* Rows in Z-order (round 6): order_dev int32 [n] = the STABLE argsort of me_coords_spatial_keys' keys, by the library's
 * own LSD radix sort (the reference sorts with thrust on its map path, src/coordinate_map_gpu.cu:766-772).  bbox: host
 * ints [2 * ncol], column minima then maxima of the rows as me_coords_insert_and_map_bbox returns them, or NULL (then
 * every key byte is sorted: eight passes instead of three for a 70^3 scene).  The tile plans of the fp32 kernels on
 * row-space tables and the halo plans are cut from this order. */
int64_t me_coords_zorder_workspace_bytes(int64_t n);
int me_coords_zorder(const int32_t *coords_dev, int64_t n, int32_t ncol, const int32_t *tensor_stride,
                     const int32_t *bbox, int32_t *order_dev, void *workspace_dev, int64_t workspace_bytes, void *stream);

/* rows[q] = row of query q in the map, or -1.  Replaces CoordinateMapGPU::find
 * (src/coordinate_map_gpu.cu:284-361). */
int me_coords_find(const uint64_t *table_dev, int64_t capacity, const int32_t *map_coords_dev,
                   int32_t ncol, const int32_t *queries_dev, int64_t nq, int32_t *rows_dev,
                   void *stream);

/* ---- kernel map (replaces CoordinateMapGPU::kernel_map, src/coordinate_map_gpu.cu:1546-1745, and
 *      gpu_kernel_map::decompose, src/kernel_map.cuh:313-405) ----------------------------------- */

/* Scratch bytes for the two kernel-map passes. */
int64_t me_kernel_map_workspace_bytes(int64_t n_out, int64_t volume);

/* Pass 1: neighbour table + per-offset pair counts.
 *   nbr_dev   int32 [volume, n_out] (out): in-map row of (out row u, offset k) or -1
 *   k_offsets host int64 [volume + 1] (out): exclusive prefix of pair counts — SYNC.  NULL (ABI 1.2): no read-back and
 *             no synchronisation; k_offsets_dev is then required and the caller allocates the pair lists at their
 *             upper bound n_out * volume (me_kernel_map_compact writes only the first k_offsets[volume] entries)
 *   k_offsets_dev int64 [volume + 1] on the device (out, may be NULL): the same prefix, for the kernels that
 *             take it as a device array (transpose, wgrad) — saves the caller a host-to-device copy
 * The iteration direction is the reference's: iterate OUTPUT coordinates, look up the INPUT map
 * (src/coordinate_map_cpu.hpp:626-649). */
int me_kernel_map_probe(const uint64_t *in_table_dev, int64_t in_capacity,
                        const int32_t *in_coords_dev, const int32_t *out_coords_dev, int64_t n_out,
                        const me_region *region, int32_t *nbr_dev, int64_t *k_offsets, int64_t *k_offsets_dev,
                        void *workspace_dev, int64_t workspace_bytes, void *stream);

/* Pass 2: wavefront ballot/prefix-sum compaction of the table into the reference's per-offset
 * pair lists (kernel_map.hpp:40-53): pairs of offset k live at [k_offsets[k], k_offsets[k+1]),
 * sorted by output row (deterministic).  Must follow me_kernel_map_probe with the same workspace. */
int me_kernel_map_compact(const int32_t *nbr_dev, int64_t n_out, int64_t volume,
                          int32_t *in_pairs_dev, int32_t *out_pairs_dev, void *workspace_dev,
                          int64_t workspace_bytes, void *stream);

/* Transposed neighbour table: nbrT[k, i] = out row paired with in row i under offset k, or -1.
 * (each (k, in row) occurs in at most one pair).   k_offsets_dev: int64 [volume+1] on device. */
int me_kernel_map_transpose(const int32_t *in_pairs_dev, const int32_t *out_pairs_dev,
                            const int64_t *k_offsets_dev, int64_t volume, int64_t n_pairs,
                            int64_t n_in, int32_t *nbrT_dev, void *stream);

/* ---- spatial index + LDS-bucketed kernel map (round 2) ---------------------------------------------------------
 * The north_star's "LDS-bucketed open-address hashing with coalesced HBM reads": the bucket of a kernel-map probe
 * is SPATIAL.  A map's rows are ordered by the supercell that contains them (<= 4096 cells: 16^3 for D = 3); a
 * workgroup owns one supercell of the query map, stages the rows of the 3^D neighbouring supercells of the lookup
 * map (contiguous ranges of its sorted coordinate array: coalesced reads, the only HBM reads of the build) into a
 * dense halo grid in LDS and answers all rows x volume probes from LDS; the neighbour table is written in POSITION
 * space (position = rank in supercell order; `order` maps positions back to rows), where a supercell is one
 * contiguous, coalesced range.  Replaces CoordinateMapGPU::kernel_map (src/coordinate_map_gpu.cu:1546-1745), whose
 * probes each walk the global table (src/3rdparty/concurrent_unordered_map.cuh:304-360). */
typedef struct me_spatial_grid {
  int32_t ncol;                        /* D + 1 */
  int32_t shift[ME_MAX_DIM];           /* log2 of the supercell side (cells of one tensor stride) per axis */
  int32_t sc_min[ME_MAX_DIM + 1];      /* [0] smallest batch index, [1 + d] smallest supercell coordinate of axis d */
  int32_t sc_dim[ME_MAX_DIM + 1];      /* extents of the dense supercell directory: batch indices, supercells per axis */
  int32_t tensor_stride[ME_MAX_DIM];   /* cell size */
} me_spatial_grid;

/* me_coords_insert_and_map that also returns the bounding box of the coordinates (host int32 [2 * ncol]: the minima
 * of the ncol columns, then the maxima) on the SAME read-back: it sizes the supercell directory without a
 * synchronisation of its own. */
int me_coords_insert_and_map_bbox(const int32_t *coords_dev, int64_t n, int32_t ncol, uint64_t *table_dev,
                                  int64_t capacity, int32_t *coords_unique_dev, int64_t *unique_map_dev,
                                  int64_t *inverse_map_dev, int64_t *n_unique, int32_t *bbox /* host, may be NULL */,
                                  void *workspace_dev, int64_t workspace_bytes, void *stream);

/* number of supercells m of the directory (product of sc_dim), -1 if invalid / too large */
int64_t me_spatial_cells(const me_spatial_grid *grid);
int64_t me_spatial_index_workspace_bytes(int64_t n, int64_t m);
/* order [n] (position -> row), pos_of_row [n], coords_sorted [n, ncol] (rows in position order), dir_start uint32
 * [m + 1] (first position of every supercell).  One key pass, ceil(log2 m / 8) stable radix passes: no host sync. */
int me_spatial_index_build(const int32_t *coords_dev, int64_t n, const me_spatial_grid *grid, int32_t *order_dev,
                           int32_t *pos_of_row_dev, int32_t *coords_sorted_dev, uint32_t *dir_start_dev,
                           void *workspace_dev, int64_t workspace_bytes, void *stream);

/* LDS bytes of the probe for this region and map pair, or -1 when it is not eligible (maps of different tensor
 * stride or supercell side, offsets reaching beyond one supercell, halo grid larger than the LDS): the caller then
 * uses me_kernel_map_probe. */
int64_t me_kernel_map_probe_lds_bytes(const me_region *region, const me_spatial_grid *query_grid,
                                      const me_spatial_grid *lookup_grid);
/* nbr_pos int32 [volume, n_q] (out): ROW of the lookup map paired with (offset k, query POSITION p), or -1.
 * k_offsets_dev int64 [volume + 1] (out, device; may be NULL): exclusive prefix of the per-offset pair counts — the
 * counts are taken inside the probe (wave ballots) and scanned into the workspace (me_kernel_map_workspace_bytes),
 * which then feeds me_kernel_map_compact_ordered.  NO host synchronisation: copy k_offsets_dev asynchronously and
 * read it when a host value is first needed. */
int me_kernel_map_probe_lds(const me_spatial_grid *query_grid, const int32_t *q_coords_sorted_dev,
                            const uint32_t *q_dir_start_dev, int64_t n_q, const me_spatial_grid *lookup_grid,
                            const int32_t *l_coords_sorted_dev, const int32_t *l_order_dev,
                            const uint32_t *l_dir_start_dev, const me_region *region, int32_t *nbr_pos_dev,
                            int64_t *k_offsets_dev, void *workspace_dev, int64_t workspace_bytes, void *stream);
/* Per-offset pair counts of an existing neighbour table (+ their prefix in the workspace for the compaction):
 * k_offsets_dev int64 [volume + 1] on the device; k_offsets (host, may be NULL: then NO synchronisation — copy
 * k_offsets_dev asynchronously and read it when first needed). */
int me_kernel_map_count(const int32_t *nbr_dev, int64_t n_out, int64_t volume, int64_t *k_offsets /* host or NULL */,
                        int64_t *k_offsets_dev, void *workspace_dev, int64_t workspace_bytes, void *stream);
/* me_kernel_map_compact for a position-space table: the target row of position p is order[p] (NULL: p itself). */
int me_kernel_map_compact_ordered(const int32_t *nbr_dev, const int32_t *order_dev, int64_t n_out, int64_t volume,
                                  int32_t *in_pairs_dev, int32_t *out_pairs_dev, void *workspace_dev,
                                  int64_t workspace_bytes, void *stream);
/* me_kernel_map_transpose into the POSITION space of the in map: nbrT[k, pos_in[in row]] = out row (pos_in NULL: the
 * row itself).  n_pairs_bound: any upper bound of the pair count (launch geometry only). */
int me_kernel_map_transpose_ordered(const int32_t *in_pairs_dev, const int32_t *out_pairs_dev,
                                    const int64_t *k_offsets_dev, int64_t volume, int64_t n_pairs_bound, int64_t n_in,
                                    const int32_t *pos_in_dev, int32_t *nbrT_dev, void *stream);

/* ---- tile plan for the target-stationary convolution ----------------------------------------- */
/* A plan cuts the target rows into tiles of `tile_rows` consecutive rows (any value in
 * [ME_GROUP_ROWS, ME_MAX_TILE_ROWS]; me_conv_plan_config picks it so that tiles x column slabs
 * fill the GPU's workgroup slots evenly).  Per tile and kernel offset k ("item") the valid
 * (k, source row) entries are padded to groups of 16 (one MFMA tile) and the groups are cut into
 * batches of at most `batch_groups` groups (dealt evenly: 5 groups -> 3 + 2); a batch is what the convolution
 * kernel stages in LDS at once and never mixes offsets. */
#define ME_GROUP_ROWS 16
#define ME_MAX_TILE_ROWS 256
#define ME_MAX_BATCH_GROUPS 4
int64_t me_plan_num_tiles(int64_t n_tgt, int32_t tile_rows);
/* int32 elements of tile_bptr_dev: 2 * num_tiles + 1 since ABI 1.2 (the tiles' batch ranges, then their dispatch
 * order).  Size the buffer with this call, not with num_tiles + 1 (the ABI 1.0 size): me_plan_build writes and every
 * me_conv_target_* reads the dispatch order behind the ranges. */
int64_t me_plan_tile_bptr_elems(int64_t n_tgt, int32_t tile_rows);
/* upper bound on the number of groups (and of batches) for a table with n_pairs valid entries; includes the four
 * groups (64 slots) that me_plan_build fills BEHIND the last group of the plan with {source row 0, dummy target row}:
 * the convolution kernels read the 64-slot index window of a batch to its end without clamping.  plan_src_dev /
 * plan_dst_dev must therefore really hold 16 * me_plan_max_groups entries. */
int64_t me_plan_max_groups(int64_t n_tgt, int64_t volume, int64_t n_pairs, int32_t tile_rows);
int64_t me_plan_workspace_bytes(int64_t n_tgt, int64_t volume, int32_t tile_rows);
/*   tbl_dev        int32 [volume, n_tgt]  neighbour table (nbr for forward, nbrT for dgrad)
 *   order_dev      int32 [n_tgt] or NULL   target rows in tile order: tile t owns the rows
 *                                          order[t*tile_rows .. (t+1)*tile_rows)  (NULL = identity;
 *                                          pass the argsort of me_coords_spatial_keys for compact tiles)
 *   plan_src_dev   int32 [16 * max_groups] (out) source row per slot, -1 = padding (the kernels gather row 0 for it;
 *                                                its products land in the dummy accumulator row)
 *   plan_dst_dev   int32 [16 * max_groups] (out) target row local to its tile; padding slots point at
 *                                                the dummy row `tile_rows`; the global target row of
 *                                                (tile t, local row d) is order[t * tile_rows + d]
 *   batch_desc_dev int32 [2 * max_groups]  (out) per batch {first group, (k << 8) | number of groups}
 *   tile_bptr_dev  int32 [me_plan_tile_bptr_elems = 2 * num_tiles + 1] (out) [0, num_tiles]: batch range of each tile; behind it the DISPATCH
 *                  ORDER of the tiles (a permutation, heaviest tile first): workgroup b of the convolution kernels
 *                  takes tile tile_bptr[num_tiles + 1 + b]
 *   item_gptr_dev  int32 [num_tiles * volume + 1] (out) first group of each (tile, k) item
 */
int me_plan_build(const int32_t *tbl_dev, const int32_t *order_dev, int64_t n_tgt, int64_t volume,
                  int32_t tile_rows, int32_t batch_groups, int32_t *plan_src_dev, int32_t *plan_dst_dev,
                  int32_t *batch_desc_dev, int32_t *tile_bptr_dev, int32_t *item_gptr_dev,
                  void *workspace_dev, int64_t workspace_bytes, void *stream);

/* Every plan of a scene at once (ABI 1.4).  A network on a NEW scene builds ~45 plans (MinkUNet34C: 10 kernel maps x
 * forward / input gradient x tile geometries); me_plan_build is 4 launches + 2 memsets each, on mostly idle hardware.
 * me_plan_build_multi walks a table of jobs in 4 launches: the arrays it writes are those of me_plan_build, bit for bit.
 * What the reference does at this point: one thrust sort + scan per kernel map (src/kernel_map.cuh:313-405).
 *   me_plan_jobs_init       fills n_tiles / n_items / item_base of every job (host) -> total items, -1: invalid geometry
 *   jobs_host / jobs_dev    the SAME initialised table in host memory (launch geometry, argument checks) and in device
 *                           memory (read by the kernels; uploaded by the caller on `stream`)
 *   workspace_dev           me_plan_multi_workspace_bytes(total items) */
typedef struct me_plan_job {
  const int32_t *tbl;       /* device: [volume, n_tgt], as me_plan_build */
  const int32_t *order;     /* device: [n_tgt] or NULL */
  int64_t n_tgt, volume;
  int32_t tile_rows, batch_groups;
  int32_t *plan_src, *plan_dst, *batch_desc, *tile_bptr, *item_gptr;   /* device (out), sized as for me_plan_build */
  int64_t n_tiles, n_items, item_base;                                  /* out of me_plan_jobs_init */
} me_plan_job;
int64_t me_plan_jobs_init(me_plan_job *jobs_host, int32_t n_jobs);
int64_t me_plan_multi_workspace_bytes(int64_t total_items);
int me_plan_build_multi(const me_plan_job *jobs_host, const me_plan_job *jobs_dev, int32_t n_jobs, void *workspace_dev,
                        int64_t workspace_bytes, void *stream);

/* ---- convolution feature kernels (replace ConvolutionForwardKernelGPU / BackwardKernelGPU,
 *      src/convolution_kernel.cu:320-496, 553-757; CPU twins src/convolution_kernel.hpp:33-144) -- */

/* Weights are handed to the convolution kernel PACKED: the register image of the MFMA operand
 * (one 16-byte element per lane and k-step quad, zero-padded to the kernel's channel tiling; layout
 * documented at k_pack_weights in csrc/conv.hip).  Pack once per call (~1 us for 0.9 MB):
 *   transposed = 0: w is [volume, c_src, c_dst]                     (forward: w = kernel)
 *   transposed = 1: w is [volume, c_dst, c_src], i.e. the FORWARD kernel when computing dgrad with
 *                   c_src = Cout, c_dst = Cin (so no separate transpose pass is needed). */
int64_t me_conv_packed_weight_elems(int64_t volume, int32_t c_src, int32_t c_dst); /* floats */
int me_conv_pack_weights_f32(const float *w_dev, int64_t volume, int32_t c_src, int32_t c_dst,
                             int32_t transposed, float *packed_dev, void *stream);

/* Target-stationary gather -> LDS -> MFMA(fp32 16x16x4) -> LDS accumulate -> one coalesced store.
 *   dst[t, :] = sum over plan entries (k, s) of tile(t):  src[s, :] @ w[k]      (w[k]: [c_src, c_dst])
 * Forward: src = in_feat, packed kernel, plan from nbr.  dgrad: src = grad_out, kernel packed with
 * transposed = 1, plan from nbrT.  Every target row is written (rows without entries get zeros).
 * The plan must have been built with the same tile_rows / batch_groups (me_conv_plan_config). */
int me_conv_target_f32(const float *src_feat_dev, int64_t n_src, int32_t c_src,
                       const float *packed_w_dev, int64_t volume, int32_t c_dst,
                       const int32_t *plan_src_dev, const int32_t *plan_dst_dev,
                       const int32_t *batch_desc_dev, const int32_t *tile_bptr_dev,
                       const int32_t *order_dev /* as given to me_plan_build, or NULL */, float *dst_feat_dev,
                       int64_t n_tgt, int32_t tile_rows, int32_t batch_groups, void *stream);

/* The same launch with MULTI-OFFSET BATCHES (round 3): runs of single-group batches of consecutive offsets — what a
 * sparse map's plan consists of — are staged and multiplied together, up to four offsets per barrier pair, each group
 * with its own offset's weight slice.  For maps with fewer than ~24 pairs per (tile, offset) item; fp32 results in a
 * fixed order (not bit-identical to me_conv_target_f32: the partial sums of a fused batch are added to the tile as a
 * whole).  Shapes without a fused instantiation (slabs of 96 columns, chunks of 96 channels, >= 4 GiB sources) and
 * plans with batch_groups < 4 (the stage buffer must hold four groups) run the plain kernel. */
int me_conv_target_f32_fused(const float *src_feat_dev, int64_t n_src, int32_t c_src, const float *packed_w_dev,
                             int64_t volume, int32_t c_dst, const int32_t *plan_src_dev, const int32_t *plan_dst_dev,
                             const int32_t *batch_desc_dev, const int32_t *tile_bptr_dev, const int32_t *order_dev,
                             float *dst_feat_dev, int64_t n_tgt, int32_t tile_rows, int32_t batch_groups, void *stream);

/* Plan geometry for a (target rows, channels) problem: the tile height is chosen so that tiles x column
 * slabs is just below a multiple of the GPU's resident-workgroup slots (a 100k-voxel layer is only
 * ~2 workgroup rounds long, so an unlucky tile count can idle a third of the chip) while the
 * accumulator tile + the stage buffer of batch_groups groups fit the 160 KiB LDS; n_pairs (density)
 * steers the trade-off against the 16-row group padding and sizes the batch. */
int me_conv_plan_config(int64_t n_tgt, int64_t volume, int64_t n_pairs, int32_t c_src, int32_t c_dst,
                        int32_t *tile_rows, int32_t *batch_groups);

/* wt[k, j, i] = w[k, i, j] */
int me_transpose_kernel_f32(const float *w_dev, int64_t volume, int32_t c_in, int32_t c_out,
                            float *wt_dev, void *stream);

/* Weight gradient: grad_w[k] = sum over pairs e of offset k of  x[in[e], :]^T (outer) dy[out[e], :]
 * (src/convolution_kernel.hpp:128-142).  The pair list is cut into equal ranges (one per workgroup,
 * regardless of offset boundaries); MFMA fp32 16x16x4 fed straight from global memory; partial
 * register images to the workspace; deterministic second-pass reduction in range order.
 *   k_offsets: host int64 [volume+1] (sizes the grid), k_offsets_dev: the same values on the device;
 *   workspace bytes from me_conv_wgrad_workspace_bytes. */
int64_t me_conv_wgrad_workspace_bytes(const int64_t *k_offsets, int64_t volume, int32_t c_in,
                                      int32_t c_out);
int me_conv_wgrad_f32(const float *x_dev, int64_t n_in /* rows of x */, int32_t c_in, const float *dy_dev,
                      int64_t n_out /* rows of dy */, int32_t c_out,
                      const int32_t *in_pairs_dev, const int32_t *out_pairs_dev,
                      const int64_t *k_offsets /* host */, const int64_t *k_offsets_dev,
                      int64_t volume, float *grad_w_dev, void *workspace_dev,
                      int64_t workspace_bytes, void *stream);

/* ---- bf16 features (fp32 accumulation) --------------------------------------------------------------
 * The reference computes in float / double only (AT_DISPATCH_FLOATING_TYPES, src/convolution_gpu.cu:137-155);
 * BASELINE configs[2] (MinkUNet34C, bf16) asks for a reduced-precision path.  Feature matrices are bf16
 * (uint16_t bit patterns, torch.bfloat16), [n, c] row-major; the SAME tile plans / pair lists are used.
 * Semantics: weights rounded to bf16 (RNE) at pack time, exact products, fp32 sums in the plan's fixed
 * order, one rounding of the result to bf16 — i.e. the fp32 convolution of the rounded operands.
 *   me_conv_pack_weights_bf16: w_is_f32 != 0: w_dev holds fp32 master weights, else bf16; layouts and
 *                              `transposed` as for me_conv_pack_weights_f32.
 *   me_conv_target_bf16:       forward / dgrad on v_mfma_f32_16x16x32_bf16 (arguments as me_conv_target_f32).
 *   me_conv_wgrad_bf16:        grad_w (fp32 out) from bf16 x / dy on v_mfma_f32_16x16x32_bf16 (rows staged in
 *                              LDS once per workgroup, operands read back transposed with
 *                              ds_read_b64_tr_b16); workspace bytes from me_conv_wgrad_workspace_bytes_bf16. */
int me_conv_plan_config_bf16(int64_t n_tgt, int64_t volume, int64_t n_pairs, int32_t c_src, int32_t c_dst,
                             int32_t *tile_rows, int32_t *batch_groups);  /* plan geometry of the bf16 kernel */
int64_t me_conv_packed_weight_elems_bf16(int64_t volume, int32_t c_src, int32_t c_dst); /* bf16 elements */
int me_conv_pack_weights_bf16(const void *w_dev, int32_t w_is_f32, int64_t volume, int32_t c_src, int32_t c_dst,
                              int32_t transposed, uint16_t *packed_dev, void *stream);
int me_conv_target_bf16(const uint16_t *src_feat_dev, int64_t n_src, int32_t c_src,
                        const uint16_t *packed_w_dev, int64_t volume, int32_t c_dst,
                        const int32_t *plan_src_dev, const int32_t *plan_dst_dev,
                        const int32_t *batch_desc_dev, const int32_t *tile_bptr_dev,
                        const int32_t *order_dev, uint16_t *dst_feat_dev,
                        int64_t n_tgt, int32_t tile_rows, int32_t batch_groups, void *stream);
/* The same operation, arguments and results (bit-identical) with BATCH FUSION: consecutive small batches of a tile —
 * up to four kernel offsets — are staged and multiplied per barrier pair.  For sparse maps, where most (tile, offset)
 * items hold a single 16-row group (a dense layer is 20 - 40 % faster on me_conv_target_bf16).  Fusion needs a stage
 * buffer of four groups: a plan with batch_groups < 4 runs as me_conv_target_bf16 does. */
int me_conv_target_bf16_fused(const uint16_t *src_feat_dev, int64_t n_src, int32_t c_src,
                              const uint16_t *packed_w_dev, int64_t volume, int32_t c_dst,
                              const int32_t *plan_src_dev, const int32_t *plan_dst_dev,
                              const int32_t *batch_desc_dev, const int32_t *tile_bptr_dev,
                              const int32_t *order_dev, uint16_t *dst_feat_dev,
                              int64_t n_tgt, int32_t tile_rows, int32_t batch_groups, void *stream);
/* The same launch (fused != 0: the batch-fusion instantiation) that ALSO leaves the batch-norm statistics of its output
 * behind: per tile and output channel the mean and M2 = sum (y - mean)^2 of the rounded values it stores, in
 * part_mean_dev / part_m2_dev [ceil(n_tgt / tile_rows)][c_dst] floats (slot = tile index, every slot written).  In the
 * reference batch norm is a separate torch operator on the feature matrix (MinkowskiEngine/MinkowskiNormalization.py:
 * 51-98); me_bn_stats_from_tiles turns these partials into its mean / rstd without reading the matrix again.
 * me_conv_stats_supported_bf16: 1 when the tile shape chosen for (c_src, c_dst) has the epilogue. */
int32_t me_conv_stats_supported_bf16(int32_t c_src, int32_t c_dst);
int me_conv_target_bf16_stats(const uint16_t *src_feat_dev, int64_t n_src, int32_t c_src,
                              const uint16_t *packed_w_dev, int64_t volume, int32_t c_dst,
                              const int32_t *plan_src_dev, const int32_t *plan_dst_dev,
                              const int32_t *batch_desc_dev, const int32_t *tile_bptr_dev,
                              const int32_t *order_dev, uint16_t *dst_feat_dev,
                              int64_t n_tgt, int32_t tile_rows, int32_t batch_groups, int32_t fused,
                              float *part_mean_dev, float *part_m2_dev, void *stream);
/* Split-K launches (round 4).  The reference runs one GEMM per kernel offset and adds into the output with atomics
 * (src/convolution_kernel.cu:320-496); here a workgroup owns a tile of target rows and walks all offsets — which on a
 * SMALL coordinate map (MinkUNet's 5k-voxel level) means 128 tiles of 39 rows that each stream the whole packed weight
 * tensor.  me_conv_plan_config_bf16_ex is me_conv_plan_config_bf16 that may also answer split_k = G > 1 with G-times
 * taller tiles: the launch then has G offset groups per tile, every workgroup walks K / G offsets, the groups' fp32
 * tiles go through `workspace_dev` (me_conv_splitk_workspace_bytes) and a second kernel adds them in group order,
 * rounds once and stores (same semantics: fp32 sums in a fixed order, one rounding; NOT the bits of the unsplit launch).
 * me_conv_target_bf16_ex is the one entry point of the bf16 forward / dgrad launch: fused / statistics / split-K by
 * argument (split_k = 1, workspace NULL, part_* NULL: me_conv_target_bf16). */
int me_conv_plan_config_bf16_ex(int64_t n_tgt, int64_t volume, int64_t n_pairs, int32_t c_src, int32_t c_dst,
                                int32_t *tile_rows, int32_t *batch_groups, int32_t *split_k);
int64_t me_conv_splitk_workspace_bytes(int64_t n_tgt, int32_t tile_rows, int32_t c_dst, int32_t split_k);
int me_conv_target_bf16_ex(const uint16_t *src_feat_dev, int64_t n_src, int32_t c_src,
                           const uint16_t *packed_w_dev, int64_t volume, int32_t c_dst,
                           const int32_t *plan_src_dev, const int32_t *plan_dst_dev,
                           const int32_t *batch_desc_dev, const int32_t *tile_bptr_dev,
                           const int32_t *order_dev, uint16_t *dst_feat_dev,
                           int64_t n_tgt, int32_t tile_rows, int32_t batch_groups, int32_t fused, int32_t split_k,
                           void *workspace_dev, float *part_mean_dev, float *part_m2_dev, void *stream);
/* Row-wise launches (round 6, csrc/conv_rowwise.hip).  For a kernel-map side on which EVERY target row has EXACTLY ONE
 * pair, dst[tgt_rows[e]] = src[src_rows[e]] @ W[k(e)] for every pair e — no sum, hence no tile plan, no LDS accumulator:
 * the x rows stream from global memory into the MFMA operand registers, W[k] comes from the packed image of
 * me_conv_pack_weights_bf16 / me_conv_pack_weights_multi (the SAME image the tile-plan launch of the layer uses; the
 * transposed image for an input gradient).  Replaces, for those sides, what me_conv_target_bf16 does:
 *   - kernel volume 1, stride 1: the reference's dense `input.F.mm(kernel)` (MinkowskiEngine/MinkowskiConvolution.py:304-308)
 *     and its input gradient;
 *   - kernel_size == stride maps (src/coordinate_map_manager.cpp:402-429 out maps): forward of
 *     ConvolutionTransposeForwardGPU (pybind/extern.hpp:99-143) and the input gradient of ConvolutionBackwardGPU
 *     (src/convolution_gpu.cu:161-244) — the fine side of the map.
 * src_rows_dev / tgt_rows_dev: the kernel map's pair lists (kernel_map.hpp:40-53 layout: pairs of an offset contiguous)
 * with the side's SOURCE rows in src_rows; k_offsets_dev int64 [volume + 1] on the device; n_pairs_bound >= the pair
 * count (the launch is sized by it; for such a side the pair count IS n_tgt).  The caller guarantees the one-pair-per-
 * row property (a row without a pair is not written, a row with two pairs is written twice).  Semantics of the tile-plan
 * launch: fp32 sums over the channels, one rounding to bf16.
 * me_conv_rowwise_supported_bf16: 1 when (volume <= 64, c_src % 8 == 0, c_dst % 8 == 0, W[k] of one 128-column slab
 * within 64 KB of LDS) the kernel takes the shape.
 * No batch-norm statistics epilogue: a layer whose statistics are wanted either stays on me_conv_target_bf16_stats or
 * is followed by the ordinary pass over its output (me_bn_stats). */
int32_t me_conv_rowwise_supported_bf16(int64_t volume, int32_t c_src, int32_t c_dst);
int me_conv_rowwise_bf16(const uint16_t *src_feat_dev, int64_t n_src, int32_t c_src, const uint16_t *packed_w_dev,
                         int64_t volume, int32_t c_dst, const int32_t *src_rows_dev, const int32_t *tgt_rows_dev,
                         const int64_t *k_offsets_dev, int64_t n_pairs_bound, uint16_t *dst_feat_dev, int64_t n_tgt,
                         void *stream);
int64_t me_conv_wgrad_workspace_bytes_bf16(const int64_t *k_offsets, int64_t volume, int32_t c_in, int32_t c_out);
int me_conv_wgrad_bf16(const uint16_t *x_dev, int64_t n_in, int32_t c_in, const uint16_t *dy_dev, int64_t n_out,
                       int32_t c_out,
                       const int32_t *in_pairs_dev, const int32_t *out_pairs_dev,
                       const int64_t *k_offsets /* host */, const int64_t *k_offsets_dev,
                       int64_t volume, float *grad_w_dev, void *workspace_dev,
                       int64_t workspace_bytes, void *stream);

/* ---- float64 features (round 4) ----------------------------------------------------------------------------------------
 * The reference instantiates its feature operators for float and double (AT_DISPATCH_FLOATING_TYPES,
 * src/convolution_gpu.cu:137-155; the pooling / broadcast units alike) and its own tests are float64 gradchecks
 * (MinkowskiEngine/utils/gradcheck.py:34-57).  csrc/f64.hip is that instantiation: plain double FMAs, one thread per
 * output element on the dense neighbour tables / pair lists, deterministic (offsets ascending, then channels) —
 * a yardstick, not a hot path.
 *   me_conv_target_f64: dst[t] = sum_k src[tbl[k][t]] @ W_k on the neighbour table tbl int32 [volume, n_tgt] (source row
 *                       of (offset, target row) or -1); w_dev is the kernel [K, c_src, c_dst], or with transposed != 0
 *                       the FORWARD kernel [K, c_dst, c_src] read transposed (input gradient).
 *   me_conv_wgrad_f64:  grad_w [K, c_in, c_out] from the pair lists (k_offsets_dev: device prefix).
 *   me_pool_*_f64, me_global_pool_f64 (no workspace), me_broadcast_f64: arguments as their _f32 twins, double rows;
 *                       counts stay float32, argmax / masks int32. */
int me_conv_target_f64(const double *src_feat_dev, int64_t n_src, int32_t c_src, const double *w_dev, int32_t transposed,
                       int64_t volume, int32_t c_dst, const int32_t *tbl_dev, double *dst_feat_dev, int64_t n_tgt,
                       void *stream);
int me_conv_wgrad_f64(const double *x_dev, int32_t c_in, const double *dy_dev, int32_t c_out, const int32_t *in_pairs_dev,
                      const int32_t *out_pairs_dev, const int64_t *k_offsets_dev, int64_t volume, double *grad_w_dev,
                      void *stream);
int me_pool_sum_f64(const double *src_dev, int32_t c, const int32_t *tbl_dev, int64_t n_tgt, int64_t volume,
                    const float *src_count_dev, int32_t average, double *dst_dev, float *dst_count_dev, void *stream);
int me_pool_max_f64(const double *src_dev, int32_t c, const int32_t *tbl_dev, int64_t n_tgt, int64_t volume,
                    double *dst_dev, int32_t *mask_dev, void *stream);
int me_pool_max_backward_f64(const double *grad_out_dev, int32_t c, const int32_t *tbl_in_dev, int64_t n_in,
                             int64_t volume, const int32_t *mask_dev, double *grad_in_dev, void *stream);
int me_global_pool_f64(const double *src_dev, const double *src2_dev, int32_t c, const int32_t *batch_row_dev, int64_t n,
                       int32_t n_batch, int32_t mode, double *dst_dev, int32_t *dst_arg_dev, float *dst_count_dev,
                       void *stream);
int me_broadcast_f64(const double *in_dev, const double *glob_dev, const int32_t *batch_row_dev, int64_t n, int32_t c,
                     int32_t multiply, double *out_dev, void *stream);

/* Output-stationary bf16 convolution (k_conv_gather_bf16): the target rows' fp32 accumulators stay in registers for
 * all kernel offsets, absent neighbours multiply as zero rows (bf16 MFMAs cost 1/16 of fp32 ones: the waste is cheaper
 * than the plan kernel's LDS accumulator traffic).  Works on a neighbour table directly — tbl int32 [volume, n_tgt]:
 * source ROW of (offset k, target position p) or -1; order (may be NULL): position -> target row — for forward (table
 * of the out side) and dgrad (table of the in side, weights packed transposed).  No tile plan.  Same semantics as
 * me_conv_target_bf16 (fp32 sums in offset order, one rounding at the store).  Channel counts: multiples of 32
 * (me_conv_gather_supported_bf16), else use me_conv_target_bf16. */
int32_t me_conv_gather_supported_bf16(int32_t c_src, int32_t c_dst);
int64_t me_conv_gather_weight_elems_bf16(int64_t volume, int32_t c_src, int32_t c_dst);
int me_conv_gather_pack_weights_bf16(const void *w_dev, int32_t w_is_f32, int64_t volume, int32_t c_src, int32_t c_dst,
                                     int32_t transposed, uint16_t *packed_dev, void *stream);
int me_conv_gather_bf16(const uint16_t *src_feat_dev, int64_t n_src, int32_t c_src, const uint16_t *packed_dev,
                        int64_t volume, int32_t c_dst, const int32_t *tbl_dev, const int32_t *order_dev,
                        uint16_t *dst_feat_dev, int64_t n_tgt, void *stream);

/* ---- bf16 convolution on a source halo staged in LDS (csrc/conv_halo.hip, ABI 1.5) ----------------------------
 * The same operation as me_conv_target_bf16 — dst[t, :] = sum over offsets k of src[tbl[k][t], :] @ w[k], fp32 sums in a
 * fixed order (per 64-channel chunk: ascending k, ascending source channel), one rounding to bf16 — on another schedule: a tile of
 * `tile_rows` target positions keeps its fp32 sums in REGISTERS for all offsets; the distinct source rows the tile
 * touches (its halo, <= s_cap of them) are staged in LDS once per channel chunk and every offset gathers from LDS;
 * absent neighbours multiply a zero row, 16-row groups without any neighbour at an offset are skipped; no barrier and
 * no read-modify-write inside the walk over the offsets.  The reference gathers, multiplies and scatter-adds once per
 * offset (src/convolution_kernel.cu:320-496).  Results are NOT the bits of me_conv_target_bf16 (there every batch
 * starts a new accumulator), they are bitwise reproducible.
 *   me_conv_halo_use_bf16     the policy: 1 when a host should run this launch side on the halo kernel (0: the tile-plan
 *                             kernel).  ME_AMD_HALO=0 | 1 | auto.  Both hosts of this repository follow it — from the
 *                             me_conv_halo_min_uses()-th launch on the same kernel-map side on (the plan costs more
 *                             than one launch saves: scenes that are not reused never build it).
 *   me_conv_halo_config_bf16  1 when the kernel is instantiated for (volume, c_src, c_dst): volume in [2, 32],
 *                             c_src % 32 == 0, c_dst in {32, 64, 96} or a multiple of 128; answers the plan geometry.
 *   me_halo_plan_build        tbl_dev int32 [volume, n_tgt] (source row of (offset, table column) or -1; nbr for forward,
 *                             nbrT for dgrad), col_order_dev int32 [n_tgt] or NULL: table column of tile position p
 *                             (NULL: p); src_pos_dev int32 [n_src] position of every SOURCE row in a spatial order of
 *                             the source map and src_order_dev int32 [n_src] its inverse (both or neither): the halo
 *                             slots are then in position order (fewer LDS bank conflicts among the rows a gather
 *                             touches together), else in row order.  Out: halo_cnt_dev int32 [tiles] distinct source
 *                             rows of each tile; halo_rows_dev int32 [tiles * s_cap] its first s_cap of them in slot
 *                             order; lidx_dev uint16
 *                             [tiles * volume * tile_rows]: 0 = no neighbour, 1 + halo slot, 0xffff = beyond s_cap;
 *                             kmask_dev uint32 [tiles * volume]: bit g = 16-row group g has a neighbour at the offset.
 *                             A tile whose halo exceeds s_cap is served by direct gathers off tbl_dev (any map works).
 *   me_conv_halo_bf16         packed_w_dev: the image of me_conv_pack_weights_bf16 for (c_src, c_dst) (transposed = 1
 *                             for dgrad); out_order_dev int32 [n_tgt] or NULL: target ROW of tile position p;
 *                             part_mean_dev / part_m2_dev [tiles][c_dst] or NULL: the batch-norm partials of
 *                             me_conv_target_bf16_stats with tile_rows = the halo tile. */
int32_t me_conv_halo_use_bf16(int64_t n_tgt, int64_t volume, int64_t n_pairs, int32_t c_src, int32_t c_dst);
int32_t me_conv_halo_min_uses(void);   /* the launch count on one kernel-map side at which a host builds the halo plan (2; forced: 1) */
int32_t me_conv_halo_config_bf16(int64_t n_tgt, int64_t volume, int64_t n_pairs, int32_t c_src, int32_t c_dst,
                                 int32_t *tile_rows, int32_t *s_cap);
int64_t me_halo_plan_num_tiles(int64_t n_tgt, int32_t tile_rows);
int me_halo_plan_build(const int32_t *tbl_dev, const int32_t *col_order_dev, const int32_t *src_pos_dev,
                       const int32_t *src_order_dev, int64_t n_tgt, int64_t volume, int32_t tile_rows, int32_t s_cap, int32_t *halo_cnt_dev, int32_t *halo_rows_dev,
                       uint16_t *lidx_dev, uint32_t *kmask_dev, void *stream);
int me_conv_halo_bf16(const uint16_t *src_feat_dev, int64_t n_src, int32_t c_src, const uint16_t *packed_w_dev,
                      int64_t volume, int32_t c_dst, const int32_t *halo_cnt_dev, const int32_t *halo_rows_dev,
                      const uint16_t *lidx_dev, const uint32_t *kmask_dev, const int32_t *tbl_dev,
                      const int32_t *col_order_dev, const int32_t *out_order_dev, uint16_t *dst_feat_dev,
                      int64_t n_tgt, int32_t tile_rows, int32_t s_cap, float *part_mean_dev, float *part_m2_dev,
                      void *stream);

/* ---- bf16 convolution with the offsets stacked into the MFMA reduction (csrc/conv_stem.hip, ABI 1.5) -------------
 * For layers with AT MOST 8 source channels (a network's stem: 3 -> 32 channels over 5^3 offsets): one MFMA step
 * multiplies FOUR offsets (4 x 8 channels = its 32-deep reduction), every neighbour row is one 16-byte load, a wave keeps
 * 16 G target rows (G = 4 under the policy: 64) x all output columns in registers over all offsets; the weights are read from the layer's OWN kernel
 * tensor (no packed image) and kept in LDS as MFMA fragments.  The reference runs one gather - GEMM - scatter launch per
 * offset (src/convolution_kernel.cu:320-496).  Semantics of me_conv_target_bf16 (weights rounded to bf16, exact products,
 * fp32 sums in a fixed order, one rounding); results are bitwise reproducible, not the bits of the tile-plan kernel.
 *   me_conv_stem_use_bf16   the policy both hosts follow: c_src <= 8, c_dst in {16, 32, 64}, volume >= 8 (ME_AMD_STEM=0 | 1);
 *                           the weight fragments of all offsets (volume rounded up to 16) share 80 KB of LDS with the
 *                           statistics: volume <= 304 / 144 / 64 for c_dst = 16 / 32 / 64
 *   me_conv_stem_tile_rows  rows per tile (256): the tile of the batch-norm partials
 *   me_conv_stem_bf16       src_feat_dev bf16 [n_src, 8] (rows padded with zeros to 8 channels, 16-byte aligned; c_src
 *                           must be 8), w_dev the kernel [volume, 8, c_dst] (transposed != 0: [volume, c_dst, 8]) in
 *                           fp32 (w_is_f32) or bf16; tbl_dev / col_order_dev / out_order_dev as me_conv_halo_bf16;
 *                            part_mean_dev / part_m2_dev [ceil(n_tgt / tile rows)][c_dst] or NULL. */
int32_t me_conv_stem_use_bf16(int64_t n_tgt, int64_t volume, int32_t c_src, int32_t c_dst);
int32_t me_conv_stem_tile_rows(void);
int me_conv_stem_bf16(const uint16_t *src_feat_dev, int64_t n_src, int32_t c_src, const void *w_dev, int32_t w_is_f32,
                      int32_t transposed, int64_t volume, int32_t c_dst, const int32_t *tbl_dev,
                      const int32_t *col_order_dev, const int32_t *out_order_dev, uint16_t *dst_feat_dev, int64_t n_tgt,
                      float *part_mean_dev, float *part_m2_dev, void *stream);

/* ---- fp32 convolution on the bf16 matrix pipe ("bf16x6" split, csrc/conv_f32x3.hip) ---------------------
 * Same contract as me_conv_target_f32 (fp32 features / weights in, fp32 out, the reference's
 * ConvolutionForwardKernelGPU / BackwardKernelGPU input gradient, src/convolution_kernel.cu:320-757, in fp32 as
 * AT_DISPATCH_FLOATING_TYPES computes it), different arithmetic unit: every operand is split exactly into three
 * bf16 terms (a = a1 + a2 + a3) and the product is rebuilt from six v_mfma_f32_16x16x32_bf16 with fp32
 * accumulation; the dropped terms are < 2^-23 |a b| per product, i.e. below one fp32 rounding.  Fixed summation
 * order (bitwise reproducible).  A non-finite FEATURE value (gathered rows, upstream gradients, the x rows of the weight
 * gradient) behaves as in fp32 arithmetic: +-inf times a weight keeps its sign, inf * 0 and opposite infinities in one
 * sum give NaN, NaN stays NaN.  A non-finite WEIGHT-side value (packed weights, the dy rows of the weight gradient)
 * makes every output it reaches NaN, where fp32 arithmetic would keep an infinity's sign (csrc/conv_common.hpp).
 * Needs c_src % 8 == 0 (me_conv_f32x3_supported); plans come from me_plan_build with the geometry of
 * me_conv_plan_config_f32x3; weights packed by me_conv_pack_weights_f32x3 (three bf16 planes). */
int32_t me_conv_f32x3_supported(int32_t c_src, int32_t c_dst);
int me_conv_plan_config_f32x3(int64_t n_tgt, int64_t volume, int64_t n_pairs, int32_t c_src, int32_t c_dst,
                              int32_t *tile_rows, int32_t *batch_groups);
int64_t me_conv_packed_weight_elems_f32x3(int64_t volume, int32_t c_src, int32_t c_dst); /* bf16 elements */
int me_conv_pack_weights_f32x3(const float *w_dev, int64_t volume, int32_t c_src, int32_t c_dst,
                               int32_t transposed, uint16_t *packed_dev, void *stream);
int me_conv_target_f32x3(const float *src_feat_dev, int64_t n_src, int32_t c_src,
                         const uint16_t *packed_w_dev, int64_t volume, int32_t c_dst,
                         const int32_t *plan_src_dev, const int32_t *plan_dst_dev,
                         const int32_t *batch_desc_dev, const int32_t *tile_bptr_dev,
                         const int32_t *order_dev, float *dst_feat_dev,
                         int64_t n_tgt, int32_t tile_rows, int32_t batch_groups, void *stream);

/* ---- backward pass of a split-fp32 layer in two launches instead of three ---------------------------------------
 * me_conv_wgrad_f32 is two launches (partial images per pair range, then their reduce into grad_w); the reduce is
 * latency-bound and leaves the GPU almost idle.  Where the layer's weight gradient is the split kernel
 * (me_conv_wgrad_is_split_f32) and its input gradient the wave-specialised me_conv_target_f32x3 kernel, the reduce
 * can ride behind the tiles of the input-gradient launch instead, on the CUs that run out of tiles first:
 *   1. me_conv_wgrad_partials_f32        (arguments of me_conv_wgrad_f32 without grad_w): the partial images only;
 *   2. me_conv_dgrad_reduce_tail_f32x3   (arguments of me_conv_target_f32x3 for the input gradient — source dy with
 *                                        c_out channels, target dx with c_in — then the pair offsets, the workspace of
 *                                        step 1 and grad_w): dx, and grad_w bit-identical to me_conv_wgrad_f32's.
 * Same stream, in this order; stream order is the only synchronisation.  n_in must be positive.
 * me_conv_dgrad_reduce_tail_supported: 1 where both kernels exist for the layer AND the tail is short enough to pay
 * (a tail workgroup owns a CU, so wide layers keep the separate reduce); 0: use the three launches. */
int32_t me_conv_wgrad_is_split_f32(int32_t c_in, int32_t c_out);
int me_conv_wgrad_partials_f32(const float *x_dev, int64_t n_in, int32_t c_in, const float *dy_dev, int64_t n_out,
                               int32_t c_out, const int32_t *in_pairs_dev, const int32_t *out_pairs_dev,
                               const int64_t *k_offsets /* host */, const int64_t *k_offsets_dev, int64_t volume,
                               void *workspace_dev, int64_t workspace_bytes, void *stream);
int32_t me_conv_dgrad_reduce_tail_supported(int32_t c_in, int32_t c_out, int64_t volume, int64_t n_pairs);
int me_conv_dgrad_reduce_tail_f32x3(const float *dy_dev, int64_t n_out, int32_t c_out, const uint16_t *packed_w_dev,
                                    int64_t volume, int32_t c_in, const int32_t *plan_src_dev,
                                    const int32_t *plan_dst_dev, const int32_t *batch_desc_dev,
                                    const int32_t *tile_bptr_dev, const int32_t *order_dev, float *dx_dev, int64_t n_in,
                                    int32_t tile_rows, int32_t batch_groups, const int64_t *k_offsets /* host */,
                                    const int64_t *k_offsets_dev, const void *workspace_dev, int64_t workspace_bytes,
                                    float *grad_w_dev, void *stream);

/* ---- weights of many layers packed by ONE launch (csrc/pack.hip) ------------------------------------------
 * The packed images above only change when the weights do (the optimizer step), not per activation: a network packs
 * all its (layer, direction) images at once instead of twice per layer and step (MinkUNet34C: 126 launches -> 1).
 * Images are bit-identical to me_conv_pack_weights_bf16 / me_conv_pack_weights_f32x3.
 *   host:   fill w / wp / volume / c_src / c_dst / transposed / w_is_f32 / mode of each job, call
 *           me_conv_pack_job_init (sets kc, nchunks, ncb, threads), build the exclusive prefix of `threads`
 *           (n_jobs + 1 int64), copy jobs and prefix to the device;
 *   device: me_conv_pack_weights_multi(jobs_dev, n_jobs, prefix_dev, prefix[n_jobs], stream).
 * c_src / c_dst are the channels of the LAUNCH the image is for (forward: Cin, Cout; input gradient: Cout, Cin with
 * transposed = 1, `w` always the reference-layout kernel[K, Cin, Cout]). */
#define ME_PACK_BF16 0    /* image of me_conv_pack_weights_bf16 (w_is_f32: fp32 master weights are rounded RNE) */
#define ME_PACK_F32X3 1   /* image of me_conv_pack_weights_f32x3 (fp32 weights, three bf16 planes) */
typedef struct me_pack_job {
  const void *w;        /* device: kernel[K, Cin, Cout] */
  void *wp;             /* device: packed image, me_conv_packed_weight_elems_{bf16,f32x3} bf16 elements, 16-byte aligned */
  int64_t volume;
  int64_t threads;      /* out: 16-byte elements (bf16) / element triples (f32x3) of the image */
  int32_t c_src, c_dst, transposed, w_is_f32, mode;
  int32_t kc, nchunks, ncb;   /* out: source-channel chunk of the tile kernel, chunks, 16-column blocks */
} me_pack_job;
int32_t me_conv_pack_chunk_bf16(int32_t c_src, int32_t c_dst);
int32_t me_conv_pack_chunk_f32x3(int32_t c_src, int32_t c_dst);
int me_conv_pack_job_init(me_pack_job *job);
int me_conv_pack_weights_multi(const me_pack_job *jobs_dev, int32_t n_jobs, const int64_t *thread_prefix_dev,
                               int64_t total_threads, void *stream);

/* ---- pooling / broadcast (replace src/pooling_avg_kernel.cu, src/pooling_max_kernel.cu,
 *      src/broadcast_kernel.cu; CPU twins src/pooling_avg_kernel.hpp:41-150,
 *      src/pooling_max_kernel.hpp:36-117, src/broadcast_kernel.hpp:35-160) ------------------------
 * All target-stationary on the dense neighbour tables of a kernel map (tbl[k, target row] -> source row
 * or -1): no atomics, no zero-fill, summation in ascending k (the reference CPU order). */

/* Local sum / average pooling, forward AND backward:
 *   dst[t, :] = sum_k src[tbl[k, t], :]                              (src_count_dev == NULL)
 *   dst[t, :] = sum_k src[s, :] / src_count[s],  s = tbl[k, t]       (average-pooling backward:
 *               src = grad_out, tbl = transposed table, src_count = num_nonzero of the forward pass)
 * `average` != 0 divides by the number of summed rows; that number is written to dst_count_dev (float
 * [n_tgt], may be NULL) — the reference's num_nonzero (src/local_pooling_cpu.cpp:104-122). */
int me_pool_sum_f32(const float *src_dev, int32_t c, const int32_t *tbl_dev, int64_t n_tgt, int64_t volume,
                    const float *src_count_dev, int32_t average, float *dst_dev, float *dst_count_dev,
                    void *stream);
/* Local max pooling forward: dst = max over k, mask[t, c] = flat index (source row * c + channel) of the
 * first maximum in k order; rows without neighbours get -FLT_MAX / -1 (src/pooling_max_kernel.hpp:73-96). */
int me_pool_max_f32(const float *src_dev, int32_t c, const int32_t *tbl_dev, int64_t n_tgt, int64_t volume,
                    float *dst_dev, int32_t *mask_dev, void *stream);
/* Local max pooling backward: grad_in[i, c] = sum of grad_out[o, c] over the outputs o = tbl_in[k, i] whose
 * mask names (i, c)  (src/pooling_max_kernel.hpp:98-117).  tbl_in: transposed table [volume, n_in]. */
int me_pool_max_backward_f32(const float *grad_out_dev, int32_t c, const int32_t *tbl_in_dev, int64_t n_in,
                             int64_t volume, const int32_t *mask_dev, float *grad_in_dev, void *stream);

/* Global pooling over the rows of each batch index (src/global_pooling_cpu.cpp:43-238).
 *   batch_row_dev int32 [n]: row of the origin map (output row) of every input row
 *   mode 0 sum, 1 average, 2 max;  src2_dev (may be NULL): multiplied element-wise before the reduction
 *   (the gradient of a broadcast multiplication);  dst [n_batch, c];  dst_arg int32 [n_batch, c] (max: flat
 *   index row * c + channel);  dst_count float [n_batch] (sum / average; may be NULL). */
int64_t me_global_pool_workspace_bytes(int64_t n, int32_t n_batch, int32_t c);
int me_global_pool_f32(const float *src_dev, const float *src2_dev, int32_t c, const int32_t *batch_row_dev,
                       int64_t n, int32_t n_batch, int32_t mode, float *dst_dev, int32_t *dst_arg_dev,
                       float *dst_count_dev, void *workspace_dev, int64_t workspace_bytes, void *stream);

/* Broadcast (src/broadcast_kernel.hpp:35-160): out[i, :] = in[i, :] (+ | *) glob[batch_row[i], :];
 * in_dev == NULL: out[i, :] = glob[batch_row[i], :] (the gradient of global sum pooling). */
int me_broadcast_f32(const float *in_dev, const float *glob_dev, const int32_t *batch_row_dev, int64_t n,
                     int32_t c, int32_t multiply, float *out_dev, void *stream);

/* bf16 feature rows (uint16_t = raw bfloat16 bits) on the same kernels: values are widened to fp32, summed /
 * compared in fp32 in the same order and rounded once at the store.  Counts and argmax masks keep their types;
 * global pooling returns fp32 [n_batch, c] (a handful of rows; the caller rounds).  The reference has no
 * reduced-precision pooling (pybind/extern.hpp:187-392 dispatches float / double only). */
int me_pool_sum_bf16(const uint16_t *src_dev, int32_t c, const int32_t *tbl_dev, int64_t n_tgt, int64_t volume,
                     const float *src_count_dev, int32_t average, uint16_t *dst_dev, float *dst_count_dev,
                     void *stream);
int me_pool_max_bf16(const uint16_t *src_dev, int32_t c, const int32_t *tbl_dev, int64_t n_tgt, int64_t volume,
                     uint16_t *dst_dev, int32_t *mask_dev, void *stream);
int me_pool_max_backward_bf16(const uint16_t *grad_out_dev, int32_t c, const int32_t *tbl_in_dev, int64_t n_in,
                              int64_t volume, const int32_t *mask_dev, uint16_t *grad_in_dev, void *stream);
int me_global_pool_bf16(const uint16_t *src_dev, const uint16_t *src2_dev, int32_t c, const int32_t *batch_row_dev,
                        int64_t n, int32_t n_batch, int32_t mode, float *dst_dev, int32_t *dst_arg_dev,
                        float *dst_count_dev, void *workspace_dev, int64_t workspace_bytes, void *stream);
int me_broadcast_bf16(const uint16_t *in_dev, const uint16_t *glob_dev, const int32_t *batch_row_dev, int64_t n,
                      int32_t c, int32_t multiply, uint16_t *out_dev, void *stream);

/* ---- channelwise (depthwise) convolution (MinkowskiChannelwiseConvolution, the reference's
 *      MinkowskiEngine/MinkowskiChannelwiseConvolution.py:184-189: plain Python, one gather / multiply / index_put
 *      per kernel offset, no native operator) ---------------------------------------------------------------------
 * Every channel has its own kernel: weight [volume, c] row-major, bias [c] (may be NULL); n_src / n_tgt: rows of the
 * source / target feature matrices.
 *   forward:  dst[t, ch] = bias[ch] + sum_k weight[k, ch] * src[tbl[k, t], ch]      tbl = nbr [volume, n_tgt]
 *   backward: dx[i, ch]  = sum_k weight[k, ch] * dy[tbl_t[k, i], ch]                 tbl_t = nbrT [volume, n_src]
 *             dweight[k, ch] = sum_i x[i, ch] * dy[tbl_t[k, i], ch],   dbias[ch] = sum_t dy[t, ch]
 * Target-stationary on the tables like pooling: every output row is written once (rows without neighbours get the bias
 * or 0), the sums over k run in ascending order, and the weight / bias gradients are a two-level reduction (per chunk
 * of source rows, then the chunks) in a fixed order, without atomics: every result is bitwise reproducible.
 * bf16 rows (uint16_t = raw bfloat16 bits) take fp32 weight and bias, accumulate in fp32 and round once at the store;
 * dweight / dbias are fp32 (double for the _f64 variants: plain double fma in the same order, no workspace needed).
 * need_dx = 0 skips dx (dx may then be NULL).  dbias NULL skips the bias gradient.  The volume may be 1 .. 65535
 * (larger: error); n_tgt = 0 launches nothing; n_src = n_tgt = 0 in the backward only zero-fills dweight / dbias.
 * Workspace of the fp32 / bf16 backward: me_cwconv_backward_workspace_bytes(n_src, volume, c) bytes. */
int me_cwconv_forward_f32(const float *src_dev, int32_t c, const float *weight_dev, const float *bias_dev,
                          const int32_t *tbl_dev, int64_t n_src, int64_t n_tgt, int64_t volume, float *dst_dev,
                          void *stream);
int me_cwconv_forward_bf16(const uint16_t *src_dev, int32_t c, const float *weight_dev, const float *bias_dev,
                           const int32_t *tbl_dev, int64_t n_src, int64_t n_tgt, int64_t volume, uint16_t *dst_dev,
                           void *stream);
int me_cwconv_forward_f64(const double *src_dev, int32_t c, const double *weight_dev, const double *bias_dev,
                          const int32_t *tbl_dev, int64_t n_src, int64_t n_tgt, int64_t volume, double *dst_dev,
                          void *stream);
int64_t me_cwconv_backward_workspace_bytes(int64_t n_src, int64_t volume, int32_t c);
int me_cwconv_backward_f32(const float *x_dev, const float *dy_dev, int32_t c, const float *weight_dev,
                           const int32_t *tbl_t_dev, int64_t n_src, int64_t n_tgt, int64_t volume, int32_t need_dx,
                           float *dx_dev, float *dweight_dev, float *dbias_dev, void *workspace_dev,
                           int64_t workspace_bytes, void *stream);
int me_cwconv_backward_bf16(const uint16_t *x_dev, const uint16_t *dy_dev, int32_t c, const float *weight_dev,
                            const int32_t *tbl_t_dev, int64_t n_src, int64_t n_tgt, int64_t volume, int32_t need_dx,
                            uint16_t *dx_dev, float *dweight_dev, float *dbias_dev, void *workspace_dev,
                            int64_t workspace_bytes, void *stream);
int me_cwconv_backward_f64(const double *x_dev, const double *dy_dev, int32_t c, const double *weight_dev,
                           const int32_t *tbl_t_dev, int64_t n_src, int64_t n_tgt, int64_t volume, int32_t need_dx,
                           double *dx_dev, double *dweight_dev, double *dbias_dev, void *workspace_dev,
                           int64_t workspace_bytes, void *stream);

/* ---- tensor fields (TensorField, SparseTensor.slice / interpolate, MinkowskiInterpolation, spmm; the reference's
 *      quantize_coordinates_kernel, field_map_kernel and interpolation_kernel, src/coordinate_map_gpu.cu:107-145,
 *      1977-2112, and its cuSPARSE coo_spmm, src/spmm.cu) ------------------------------------------------------------
 * Field coordinates x: [n, ncol] contiguous, float32 (_f32) or float64 (_f64), column 0 the batch index.
 * tensor_stride: host int32 [ncol - 1], every entry > 0 (NULL: all 1).  ncol in [2, 8].
 * Quantisation of point i: (lrint(x[i, 0]), floor(x[i, j] / s_j) * s_j) — a division, as the reference's kernel.
 *
 * me_field_quantize_*: out int32 [n, ncol] (feed it to me_coords_insert_and_map).  No sync.
 * me_field_lookup_*: quantise and probe a map (table / capacity / map_coords as me_coords_find; 16-byte aligned for
 *   ncol 4): (sparse_rows[k], field_rows[k]) for the points whose voxel is present, in ascending field row order;
 *   sparse_rows / field_rows int32 [n] (first *n_hit valid).  SYNC (one 4-byte copy for *n_hit).
 *   Workspace: me_field_lookup_workspace_bytes(n).
 * me_field_interp_map_*: trilinear interpolation map of the points on a map of tensor stride s.  Corner v of point p
 *   (v in [0, 2^D)): bit (D - j) of v selects floor(x_j / s_j) * s_j + s_j in column j, else floor(x_j / s_j) * s_j;
 *   batch lrint(x_0).  Every present corner gives an entry (in_rows = map row, out_rows = p,
 *   weights = prod_{j=1..D} (1 - |x_j - c_j| / s_j), in the coordinate type, j ascending); entries ordered by (p, v)
 *   ascending (the reference's order after its stable remove_if).  in_rows / out_rows int32 and weights [n * 2^D]
 *   (first *nnz valid); rowptr int32 [n + 1]: entries of point p at [rowptr[p], rowptr[p + 1]).  n * 2^D < 2^31.
 *   SYNC (one 4-byte copy for *nnz).  Workspace: me_field_interp_workspace_bytes(n, ncol).
 * me_csr_from_coo: rows of a COO matrix by keys[e] in [0, n_rows), stable in entry order (the library's radix sort):
 *   rowptr int32 [n_rows + 1], cols_out[i] = cols[e_i] (cols NULL: e_i itself), vals_out[i] = vals[e_i] (val_bytes 4
 *   or 8; vals NULL: none) for the entries e_0 < e_1 < ... of each row in turn.  nnz, n_rows < 2^31.  No sync.
 *   Workspace: me_csr_from_coo_workspace_bytes(nnz).
 * me_csr_gather_*: y[r] = scale[r] * sum_{e in [rowptr[r], rowptr[r + 1])} w[e] * x[col[e]] for r < n_rows; x and y
 *   [*, c] contiguous, every col[e] a row of x.  w NULL: unweighted; scale NULL: 1.  The sum runs in entry order in fp32
 *   (fma with weights) for fp32 and bf16 features (bf16 rounds once at the store; w and scale fp32) and in double for
 *   float64 (w and scale double); rows without entries are written as zeros; no atomics, bitwise reproducible.
 *   No sync, no workspace. */
int me_field_quantize_f32(const float *x_dev, int64_t n, int32_t ncol, const int32_t *tensor_stride, int32_t *out_dev,
                          void *stream);
int me_field_quantize_f64(const double *x_dev, int64_t n, int32_t ncol, const int32_t *tensor_stride, int32_t *out_dev,
                          void *stream);
int64_t me_field_lookup_workspace_bytes(int64_t n);
int me_field_lookup_f32(const float *x_dev, int64_t n, int32_t ncol, const int32_t *tensor_stride,
                        const uint64_t *table_dev, int64_t capacity, const int32_t *map_coords_dev,
                        int32_t *sparse_rows_dev, int32_t *field_rows_dev, int64_t *n_hit, void *workspace_dev,
                        int64_t workspace_bytes, void *stream);
int me_field_lookup_f64(const double *x_dev, int64_t n, int32_t ncol, const int32_t *tensor_stride,
                        const uint64_t *table_dev, int64_t capacity, const int32_t *map_coords_dev,
                        int32_t *sparse_rows_dev, int32_t *field_rows_dev, int64_t *n_hit, void *workspace_dev,
                        int64_t workspace_bytes, void *stream);
int64_t me_field_interp_workspace_bytes(int64_t n, int32_t ncol);
int me_field_interp_map_f32(const float *x_dev, int64_t n, int32_t ncol, const int32_t *tensor_stride,
                            const uint64_t *table_dev, int64_t capacity, const int32_t *map_coords_dev,
                            int32_t *in_rows_dev, int32_t *out_rows_dev, float *weights_dev, int32_t *rowptr_dev,
                            int64_t *nnz, void *workspace_dev, int64_t workspace_bytes, void *stream);
int me_field_interp_map_f64(const double *x_dev, int64_t n, int32_t ncol, const int32_t *tensor_stride,
                            const uint64_t *table_dev, int64_t capacity, const int32_t *map_coords_dev,
                            int32_t *in_rows_dev, int32_t *out_rows_dev, double *weights_dev, int32_t *rowptr_dev,
                            int64_t *nnz, void *workspace_dev, int64_t workspace_bytes, void *stream);
/* me_field_origin_rows_f32: rows[i] = row of the origin map (tensor stride 0; table / capacity / origin_coords as
 *   me_coords_find) whose batch index is lrint(x[i, 0]), or -1: the row table of global pooling and broadcast over a
 *   field (CoordinateMapManager::origin_field_map, src/coordinate_map_gpu.cu:894-975).  rows int32 [n].  No sync. */
int me_field_origin_rows_f32(const float *x_dev, int64_t n, int32_t ncol, const uint64_t *table_dev, int64_t capacity,
                             const int32_t *origin_coords_dev, int32_t *rows_dev, void *stream);
int64_t me_csr_from_coo_workspace_bytes(int64_t nnz);
int me_csr_from_coo(const int32_t *keys_dev, const int32_t *cols_dev, const void *vals_dev, int32_t val_bytes,
                    int64_t nnz, int64_t n_rows, int32_t *rowptr_dev, int32_t *cols_out_dev, void *vals_out_dev,
                    void *workspace_dev, int64_t workspace_bytes, void *stream);
int me_csr_gather_f32(const float *x_dev, int32_t c, const int32_t *rowptr_dev, const int32_t *col_dev,
                      const float *w_dev, const float *scale_dev, int64_t n_rows, float *y_dev, void *stream);
int me_csr_gather_bf16(const uint16_t *x_dev, int32_t c, const int32_t *rowptr_dev, const int32_t *col_dev,
                       const float *w_dev, const float *scale_dev, int64_t n_rows, uint16_t *y_dev, void *stream);
int me_csr_gather_f64(const double *x_dev, int32_t c, const int32_t *rowptr_dev, const int32_t *col_dev,
                      const double *w_dev, const double *scale_dev, int64_t n_rows, double *y_dev, void *stream);

/* Direct max pooling (src/direct_max_pool.cpp, src/pooling_max_kernel.cu:55-234; ABI 1.11): entry e of the pair list says
 * "row in_map[e] of in_feat [in_nrows, c] belongs to output row out_map[e]".  For every output row o with an entry and
 * every channel: out_feat[o, ch] = max of in_feat[in_map[e], ch] over the entries with out_map[e] == o, compared as the
 * reference does (`max < cur`, from the row's first entry, entries in map order: among equal values the first entry wins;
 * bf16 compares in fp32 and stores the winner's bits), max_index[o, ch] = in_map[e*] * c + ch.  Rows without an entry:
 * out_feat 0, max_index the index type's maximum (the reference's "unused" marker).
 *   in_map / out_map: [nmap], both int32 (index_bytes 4) or both int64 (8); NOT written (the reference sorts them in
 *   place).  max_index [out_nrows, c] has the index type.  is_sorted != 0: out_map is ascending, no sort (checked).
 *   Errors: a map value outside [0, in_nrows) / [0, out_nrows) (this covers "more distinct outputs than out_nrows"),
 *   out_map not ascending under is_sorted, in_nrows * c >= 2^31 with int32 maps.  nmap, in_nrows, out_nrows < 2^31.
 *   SYNC (one 4-byte copy: the verdict of the map check).  Workspace: me_direct_max_pool_workspace_bytes(nmap, out_nrows).
 * me_direct_max_pool_backward_*: grad_in [in_nrows, c] = 0, plus grad_out[o, ch] at every max_index[o, ch] in
 *   [0, in_nrows * c) (anything else, the marker included, is skipped).  The flat indices are sorted (stable) and every run
 *   of equal indices is summed in ascending (o, ch) order by one thread (fp32 sums for bf16, one rounding): no
 *   floating-point atomics, bitwise reproducible.  out_nrows * c < 2^31, in_nrows * c < 2^32 - 1.  No sync.
 *   Workspace: me_direct_max_pool_backward_workspace_bytes(out_nrows, c). */
int64_t me_direct_max_pool_workspace_bytes(int64_t nmap, int64_t out_nrows);
int me_direct_max_pool_f32(const float *in_feat_dev, int32_t c, const void *in_map_dev, const void *out_map_dev,
                           int32_t index_bytes, int64_t nmap, int64_t in_nrows, int64_t out_nrows, int32_t is_sorted,
                           float *out_feat_dev, void *max_index_dev, void *workspace_dev, int64_t workspace_bytes,
                           void *stream);
int me_direct_max_pool_bf16(const uint16_t *in_feat_dev, int32_t c, const void *in_map_dev, const void *out_map_dev,
                            int32_t index_bytes, int64_t nmap, int64_t in_nrows, int64_t out_nrows, int32_t is_sorted,
                            uint16_t *out_feat_dev, void *max_index_dev, void *workspace_dev, int64_t workspace_bytes,
                            void *stream);
int me_direct_max_pool_f64(const double *in_feat_dev, int32_t c, const void *in_map_dev, const void *out_map_dev,
                           int32_t index_bytes, int64_t nmap, int64_t in_nrows, int64_t out_nrows, int32_t is_sorted,
                           double *out_feat_dev, void *max_index_dev, void *workspace_dev, int64_t workspace_bytes,
                           void *stream);
int64_t me_direct_max_pool_backward_workspace_bytes(int64_t out_nrows, int32_t c);
int me_direct_max_pool_backward_f32(const float *grad_out_dev, const void *max_index_dev, int32_t index_bytes,
                                    int64_t out_nrows, int32_t c, int64_t in_nrows, float *grad_in_dev,
                                    void *workspace_dev, int64_t workspace_bytes, void *stream);
int me_direct_max_pool_backward_bf16(const uint16_t *grad_out_dev, const void *max_index_dev, int32_t index_bytes,
                                     int64_t out_nrows, int32_t c, int64_t in_nrows, uint16_t *grad_in_dev,
                                     void *workspace_dev, int64_t workspace_bytes, void *stream);
int me_direct_max_pool_backward_f64(const double *grad_out_dev, const void *max_index_dev, int32_t index_bytes,
                                    int64_t out_nrows, int32_t c, int64_t in_nrows, double *grad_in_dev,
                                    void *workspace_dev, int64_t workspace_bytes, void *stream);

/* Arithmetic across coordinate maps (MinkowskiTensor._binary_functor, MinkowskiTensor.py:511-546; csrc/union_arith.hip,
 * ABI 1.12): out [nu, c] = a [na, c] (op) b [nb, c] on the union of the two maps.  Row tables, all int32:
 * a_of_u / b_of_u [nu] = the row of a / b that lies on union row u, -1 = none; u_of_a [na] / u_of_b [nb] = the union row of
 * every input row.
 *   me_union_tables:  builds the four tables from the union rows of the inputs as union_map returns them (int64 [na],
 *                     [nb], values in [0, nu); coordinates unique within an input).  A value outside [0, nu) becomes -1
 *                     in u_of_* and is not scattered.  No sync, no workspace.
 *   me_union_arith_*: every row of out is written exactly once with vector stores (16 bytes along c when c and the
 *                     pointers allow): fn(a, b) where both hold the row, the row of `a` unchanged where only a holds it
 *                     (for * and / as well), fn(0, b) where only b holds it, which is b, -b, 0 * b, 0 / b (NaN where b
 *                     is 0).  No zero fill, no atomics, independent of the launch geometry: bitwise reproducible.  bf16
 *                     combines in fp32 and rounds once.  Traffic: (na + nb + nu) * c * sizeof + 8 * nu bytes.
 *   me_union_arith_backward_*: grad_a [na, c] and / or grad_b [nb, c] (NULL: not wanted, no launch): a gather of
 *                     grad_out [nu, c] through u_of_a / u_of_b times the local derivative.  grad_a = g, g, g * b, g / b
 *                     on shared rows and g elsewhere; grad_b = g, -g, g * x, -g * ((x / b) / b) with x = a's row or 0.
 *                     a / b / a_of_u / b_of_u are read only where the operator needs them (NULL allowed for + and -).
 *   Row counts < 2^31.  No sync. */
#define ME_UNION_ADD 0
#define ME_UNION_SUB 1
#define ME_UNION_MUL 2
#define ME_UNION_DIV 3
int me_union_tables(const int64_t *a_union_dev, int64_t na, const int64_t *b_union_dev, int64_t nb, int64_t nu,
                    int32_t *u_of_a_dev, int32_t *u_of_b_dev, int32_t *a_of_u_dev, int32_t *b_of_u_dev, void *stream);
int me_union_arith_f32(const float *a_dev, const float *b_dev, int32_t c, const int32_t *a_of_u_dev,
                       const int32_t *b_of_u_dev, int64_t na, int64_t nb, int64_t nu, int32_t op, float *out_dev,
                       void *stream);
int me_union_arith_bf16(const uint16_t *a_dev, const uint16_t *b_dev, int32_t c, const int32_t *a_of_u_dev,
                        const int32_t *b_of_u_dev, int64_t na, int64_t nb, int64_t nu, int32_t op, uint16_t *out_dev,
                        void *stream);
int me_union_arith_f64(const double *a_dev, const double *b_dev, int32_t c, const int32_t *a_of_u_dev,
                       const int32_t *b_of_u_dev, int64_t na, int64_t nb, int64_t nu, int32_t op, double *out_dev,
                       void *stream);
int me_union_arith_backward_f32(const float *grad_out_dev, const float *a_dev, const float *b_dev, int32_t c,
                                const int32_t *u_of_a_dev, const int32_t *u_of_b_dev, const int32_t *a_of_u_dev,
                                const int32_t *b_of_u_dev, int64_t na, int64_t nb, int64_t nu, int32_t op,
                                float *grad_a_dev, float *grad_b_dev, void *stream);
int me_union_arith_backward_bf16(const uint16_t *grad_out_dev, const uint16_t *a_dev, const uint16_t *b_dev, int32_t c,
                                 const int32_t *u_of_a_dev, const int32_t *u_of_b_dev, const int32_t *a_of_u_dev,
                                 const int32_t *b_of_u_dev, int64_t na, int64_t nb, int64_t nu, int32_t op,
                                 uint16_t *grad_a_dev, uint16_t *grad_b_dev, void *stream);
int me_union_arith_backward_f64(const double *grad_out_dev, const double *a_dev, const double *b_dev, int32_t c,
                                const int32_t *u_of_a_dev, const int32_t *u_of_b_dev, const int32_t *a_of_u_dev,
                                const int32_t *b_of_u_dev, int64_t na, int64_t nb, int64_t nu, int32_t op,
                                double *grad_a_dev, double *grad_b_dev, void *stream);

/* Generative / expanding convolutions (CoordinateMapCPU::stride_region, src/coordinate_map_cpu.hpp:446-487;
 * manager: src/coordinate_map_manager.cpp:436-466): candidate output coordinates = every kernel offset of the
 * region around every input coordinate, candidate (row, k) at out[row * volume + k]; a following
 * me_coords_insert_and_map removes the duplicates (first occurrence wins).  region->tensor_stride holds the
 * OUTPUT tensor stride, as the reference's kernel region does.  align_stride (may be NULL) with `aligned`
 * (uint8 [n * volume]): marks the candidates whose spatial coordinates are multiples of align_stride (the
 * non-transposed expand_coordinates case keeps only those, :478-483). */
int me_coords_expand_region(const int32_t *coords_dev, int64_t n, int32_t ncol, const me_region *region,
                            const int32_t *align_stride, int32_t *out_coords_dev, uint8_t *aligned_dev,
                            void *stream);

/* ---- input pipeline on the device --------------------------------------------------
 * Voxelisation = me_coords_insert_and_map (unique_map / inverse_map) plus these two reductions.
 * Labels (src/quantization.cpp:140-196, quantize_label): colabels[u] = label of the voxel's first point,
 * or ignore_label if any point of the voxel carries a different label.  (The reference writes the
 * ignore label to colabels[inverse_mapping[u]] instead of colabels[u] — src/quantization.cpp:189 — which
 * marks the wrong voxel whenever duplicates precede row u; the intended semantics are implemented.) */
int me_coords_quantize_labels(const int64_t *unique_map_dev, int64_t n_unique, const int64_t *inverse_map_dev,
                              const int32_t *labels_dev, int64_t n, int32_t ignore_label,
                              int32_t *colabels_dev, void *stream);
/* Features of duplicate coordinates (SparseTensorQuantizationMode UNWEIGHTED_SUM / UNWEIGHTED_AVERAGE,
 * MinkowskiSparseTensor.py:317-341; the reference goes through cuSPARSE coo_spmm, src/spmm.cu):
 * dst[s, :] = sum (or mean) of src[perm[i], :] for i in [seg_offsets[s], seg_offsets[s+1]) in that order. */
int me_segment_sum_f32(const float *src_dev, int32_t c, const int64_t *perm_dev, const int64_t *seg_offsets_dev,
                       int64_t n_seg, int32_t average, float *dst_dev, void *stream);

/* ---- batch normalisation over feature rows (MinkowskiBatchNorm = torch.nn.BatchNorm1d on the feature matrix,
 *      MinkowskiEngine/MinkowskiNormalization.py:35-82; 62 of them per MinkUNet34C pass) ----
 * x / y / dy / dx: [n, c] row-major, fp32 (is_bf16 = 0) or bf16 (is_bf16 = 1); statistics and parameters fp32.
 *   me_bn_stats:    per-channel mean and rstd = 1 / sqrt(biased variance + eps) of the batch; when running_mean /
 *                   running_var are given they are updated as torch does (momentum, unbiased variance).
 *                   Two-level reduction in a fixed order (Chan's combination of per-chunk mean / M2): bitwise
 *                   reproducible.
 *   me_bn_apply:    y = (x - mean) * rstd * gamma + beta        (gamma / beta may be NULL); relu != 0: y = max(y, 0)
 *   me_bn_backward: grad_beta = sum dy, grad_gamma = sum dy * xhat,
 *                   dx = gamma * rstd * (dy - grad_beta / n - xhat * grad_gamma / n)   (training-mode gradient);
 *                   relu != 0: dy is first masked where the forward output (recomputed from x) was not positive
 *                   (batch norm + ReLU fused: MinkowskiBatchNorm followed by MinkowskiReLU in the reference)
 * workspace bytes for stats and backward: me_bn_workspace_bytes(n, c). */
int64_t me_bn_workspace_bytes(int64_t n, int32_t c);
int me_bn_stats(const void *x_dev, int32_t is_bf16, int64_t n, int32_t c, float eps, float momentum,
                float *mean_dev, float *rstd_dev, float *running_mean_dev, float *running_var_dev,
                int64_t *num_batches_tracked_dev /* may be NULL; += 1 (torch's BatchNorm buffer) */,
                void *workspace_dev, int64_t workspace_bytes, void *stream);
int me_bn_apply(const void *x_dev, int32_t is_bf16, int64_t n, int32_t c, const float *mean_dev,
                const float *rstd_dev, const float *gamma_dev, const float *beta_dev, int32_t relu, void *y_dev,
                void *stream);
int me_bn_backward(const void *x_dev, const void *dy_dev, int32_t is_bf16, int64_t n, int32_t c,
                   const float *mean_dev, const float *rstd_dev, const float *gamma_dev, const float *beta_dev,
                   int32_t relu, void *dx_dev, float *grad_gamma_dev, float *grad_beta_dev, void *workspace_dev,
                   int64_t workspace_bytes, void *stream);
/* Statistics of a matrix whose per-tile (mean, M2) partials a convolution already wrote (me_conv_target_bf16_stats):
 * tile g = rows [g * tile_rows, min((g + 1) * tile_rows, n)), partials [ceil(n / tile_rows)][c] floats each.  Same
 * outputs and running-statistics update as me_bn_stats, without reading the matrix (one small launch). */
int me_bn_stats_from_tiles(const float *part_mean_dev, const float *part_m2_dev, int64_t n, int32_t c,
                           int32_t tile_rows, float eps, float momentum, float *mean_dev, float *rstd_dev,
                           float *running_mean_dev, float *running_var_dev, int64_t *num_batches_tracked_dev,
                           void *stream);
/* Residual form (a ResNet block's `relu(bn(conv(x)) + skip)`): y = [relu] (T(x * a + b) + skip) in one pass, bit-identical
 * to me_bn_apply followed by an addition and a ReLU; the backward pass masks dy where the stored output `yout` is not
 * positive (relu != 0), writes the masked gradient to dskip (the residual branch's gradient; may be NULL) and dx. */
int me_bn_apply_residual(const void *x_dev, const void *skip_dev, int32_t is_bf16, int64_t n, int32_t c,
                         const float *mean_dev, const float *rstd_dev, const float *gamma_dev, const float *beta_dev,
                         int32_t relu, void *y_dev, void *stream);
int me_bn_backward_residual(const void *x_dev, const void *dy_dev, const void *yout_dev, int32_t is_bf16, int64_t n,
                            int32_t c, const float *mean_dev, const float *rstd_dev, const float *gamma_dev,
                            const float *beta_dev, int32_t relu, void *dx_dev, void *dskip_dev, float *grad_gamma_dev,
                            float *grad_beta_dev, void *workspace_dev, int64_t workspace_bytes, void *stream);

/* ---- synchronised batch norm (MinkowskiSyncBatchNorm, MinkowskiEngine/MinkowskiNormalization.py:85-191: batch statistics
 *      over the rows of ALL ranks of a process group; ABI 1.14): the same row passes with one more level around them.  The caller
 *      owns the exchange (one all-gather per direction); these entry points are what runs before and after it.
 * A rank's RECORD is me_bn_moments_floats(c) = 2 + 2c floats: the int64 row count (its bit pattern in the first two
 * floats — never a rounded float), mean[c], M2[c] = sum (x - mean)^2.  Records must be 8-byte aligned.
 *   me_bn_local_moments:      the record of this rank's [n, c] matrix: k_bn_partial's chunks merged in me_bn_stats' fixed
 *                             order.  Writes the record and nothing else (no rstd, no running statistics).  n = 0 is
 *                             legal (an empty rank): no row kernel, count 0, mean 0, M2 0.
 *   me_bn_stats_from_moments: moments_dev = the records of `world` ranks, [world][2 + 2c] floats in rank order (what an
 *                             all-gather leaves).  me_bn_stats' merge with the ranks as chunks, each with the count of
 *                             its record, shifted to the mean of the FIRST rank that has rows (an empty rank 0 must not
 *                             turn the shift into 0: B - A^2 / N would cancel for |mean| >> std).  Outputs as me_bn_stats;
 *                             the running statistics use the GLOBAL count (unbiased variance: N_total - 1); when no
 *                             rank has a row they stay untouched and num_batches_tracked is not incremented.
 *                             n_total_dev (may be NULL) receives the global row count.
 *                             One wave per channel, lane l takes ranks l, l + 64, ..., then a fixed tree: every rank
 *                             computes bit-identical mean / rstd.  One record gives the bits of me_bn_stats while the
 *                             row count is exact in fp32 (n <= 2^24): beyond it me_bn_stats' sum of float chunk counts
 *                             and the record's int64 count converted once may round differently.
 *   me_bn_backward_sums:      sum_dy[c] = sum dy, sum_dyx[c] = sum dy * xhat over this rank's rows (dy masked first when
 *                             relu != 0: by the output recomputed from x, or by yout_dev when it is given — the residual
 *                             form), i.e. me_bn_backward / me_bn_backward_residual stopped before the apply.  These LOCAL
 *                             sums are grad_beta / grad_gamma of the rank.  n = 0 writes zeros.
 *   me_bn_backward_reduce:    sums_dev = [world][2][c] floats in rank order (each rank's sum_dy | sum_dyx, gathered);
 *                             added per channel in rank order (lane l takes ranks l, l + 64, ..., fixed tree) — not an
 *                             all-reduce, whose order is the backend's.
 *   me_bn_backward_apply:     dx (and dskip, may be NULL) of this rank's n_local rows from the global sums:
 *                             dx = gamma * rstd * (dy - sum_dy / N - xhat * sum_dyx / N) with N = *n_total_dev when that
 *                             is given (the count me_bn_stats_from_moments left on the device), else n_total.
 *                             yout_dev != NULL with relu != 0: the residual form.  n_local = 0 launches nothing.
 * workspace bytes for me_bn_local_moments / me_bn_backward_sums: me_bn_workspace_bytes(n, c). */
int64_t me_bn_moments_floats(int32_t c);
int me_bn_local_moments(const void *x_dev, int32_t is_bf16, int64_t n, int32_t c, float *moments_dev,
                        void *workspace_dev, int64_t workspace_bytes, void *stream);
int me_bn_stats_from_moments(const float *moments_dev, int32_t world, int32_t c, float eps, float momentum,
                             float *mean_dev, float *rstd_dev, float *running_mean_dev, float *running_var_dev,
                             int64_t *num_batches_tracked_dev, int64_t *n_total_dev, void *stream);
int me_bn_backward_sums(const void *x_dev, const void *dy_dev, const void *yout_dev, int32_t is_bf16, int64_t n,
                        int32_t c, const float *mean_dev, const float *rstd_dev, const float *gamma_dev,
                        const float *beta_dev, int32_t relu, float *sum_dy_dev, float *sum_dyx_dev,
                        void *workspace_dev, int64_t workspace_bytes, void *stream);
int me_bn_backward_reduce(const float *sums_dev, int32_t world, int32_t c, float *sum_dy_dev, float *sum_dyx_dev,
                          void *stream);
int me_bn_backward_apply(const void *x_dev, const void *dy_dev, const void *yout_dev, int32_t is_bf16, int64_t n_local,
                         int64_t n_total, const int64_t *n_total_dev, int32_t c, const float *mean_dev,
                         const float *rstd_dev, const float *gamma_dev, const float *beta_dev, int32_t relu,
                         const float *sum_dy_dev, const float *sum_dyx_dev, void *dx_dev, void *dskip_dev,
                         void *stream);

/* ---- instance normalisation over feature rows (MinkowskiInstanceNorm / MinkowskiStableInstanceNorm,
 *      MinkowskiEngine/MinkowskiNormalization.py:194-399: there a chain of global poolings and broadcasts; here batch
 *      norm's pipeline with the statistics segmented by the batch index of each row; csrc/instance_norm.hip, ABI 1.9) ----
 * x / y / dy / dx: [n, c] row-major, fp32 (is_bf16 = 0) or bf16 (is_bf16 = 1: rows widened to fp32, one rounding at the
 * store); batch_row: int32 [n], the instance (origin-map row) of every row, values in [0, n_batch), rows of an instance
 * in ANY order; mean / rstd: fp32 [n_batch, c]; gamma / beta / grad_gamma / grad_beta: fp32 [c].
 *   me_inorm_stats:    mean[b] and rstd[b] = 1 / sqrt(biased variance of instance b + eps) per channel.  Two-level
 *                      reduction in a fixed order: per (chunk of rows, instance) count / mean / M2 from shifted sums,
 *                      merged with Chan's formula; bitwise reproducible.  An instance without rows: mean = 0,
 *                      rstd = 1 / sqrt(eps).
 *   me_inorm_apply:    y[i] = (x[i] - mean[b_i]) * rstd[b_i] * gamma + beta          (gamma / beta may be NULL: 1 / 0)
 *   me_inorm_backward: with xhat = (x - mean[b]) * rstd[b]: t1[b] = sum_{i in b} dy, t2[b] = sum_{i in b} dy * xhat,
 *                      dx[i] = gamma * rstd[b_i] * (dy[i] - t1[b_i] / n_b - xhat[i] * t2[b_i] / n_b),
 *                      grad_beta = sum_b t1[b], grad_gamma = sum_b t2[b] (ascending b).  gamma may be NULL (1); dx,
 *                      grad_gamma and grad_beta may each be NULL (skipped).  No atomics on values: reproducible.
 * workspace bytes for stats and backward (either precision): me_inorm_workspace_bytes(n, n_batch, c); about
 * 8 * min(512, n / 4) * n_batch * c bytes of per-chunk partials.  The _f64 entry points are the same formulae in plain double (parameters and statistics
 * double as well): the yardstick of gradcheck, not a hot path. */
int64_t me_inorm_workspace_bytes(int64_t n, int32_t n_batch, int32_t c);
int me_inorm_stats(const void *x_dev, int32_t is_bf16, const int32_t *batch_row_dev, int64_t n, int32_t n_batch,
                   int32_t c, float eps, float *mean_dev, float *rstd_dev, void *workspace_dev,
                   int64_t workspace_bytes, void *stream);
int me_inorm_apply(const void *x_dev, int32_t is_bf16, const int32_t *batch_row_dev, int64_t n, int32_t n_batch,
                   int32_t c, const float *mean_dev, const float *rstd_dev, const float *gamma_dev,
                   const float *beta_dev, void *y_dev, void *stream);
int me_inorm_backward(const void *x_dev, const void *dy_dev, int32_t is_bf16, const int32_t *batch_row_dev, int64_t n,
                      int32_t n_batch, int32_t c, const float *mean_dev, const float *rstd_dev, const float *gamma_dev,
                      void *dx_dev, float *grad_gamma_dev, float *grad_beta_dev, void *workspace_dev,
                      int64_t workspace_bytes, void *stream);
int me_inorm_stats_f64(const double *x_dev, const int32_t *batch_row_dev, int64_t n, int32_t n_batch, int32_t c,
                       double eps, double *mean_dev, double *rstd_dev, void *stream);
int me_inorm_apply_f64(const double *x_dev, const int32_t *batch_row_dev, int64_t n, int32_t n_batch, int32_t c,
                       const double *mean_dev, const double *rstd_dev, const double *gamma_dev, const double *beta_dev,
                       double *y_dev, void *stream);
int me_inorm_backward_f64(const double *x_dev, const double *dy_dev, const int32_t *batch_row_dev, int64_t n,
                          int32_t n_batch, int32_t c, const double *mean_dev, const double *rstd_dev,
                          const double *gamma_dev, double *dx_dev, double *grad_gamma_dev, double *grad_beta_dev,
                          void *workspace_dev, int64_t workspace_bytes, void *stream);

/* ---- group normalisation over feature rows (MinkowskiGroupNorm; torch.nn.GroupNorm's arithmetic applied to every
 *      instance of a sparse tensor on its own.  Instance norm's pipeline plus a merge over the channels of a group;
 *      csrc/group_norm.hip, ABI 1.15) ----
 * Arguments as for instance normalisation, plus `groups`: c % groups == 0, group g holds the cg = c / groups channels
 * [g * cg, (g + 1) * cg).  mean / rstd: fp32 [n_batch, groups]; gamma / beta / grad_gamma / grad_beta: fp32 [c].
 *   me_gnorm_stats:    mean[b, g] and rstd[b, g] = 1 / sqrt(biased variance + eps) over the n_b * cg values of instance b
 *                      in group g.  Per (chunk of rows, instance, channel) count / mean / M2 from shifted sums, merged over
 *                      the chunks with Chan's formula, then over the cg channel records of the group in ascending channel
 *                      order (equal counts: M2_g = sum M2_c + n_b * sum (mean_c - mean_g)^2).  E[x^2] - E[x]^2 is never
 *                      formed.  Fixed order, bitwise reproducible.  An instance without rows: mean = 0,
 *                      rstd = 1 / sqrt(eps).
 *   me_gnorm_apply:    y[i, ch] = (x[i, ch] - mean[b_i, g_ch]) * rstd[b_i, g_ch] * gamma[ch] + beta[ch]
 *                      (gamma / beta may be NULL: 1 / 0)
 *   me_gnorm_backward: with xhat = (x - mean) * rstd and m = n_b * cg: t1[b, ch] = sum_{i in b} dy, t2[b, ch] =
 *                      sum_{i in b} dy * xhat, grad_beta = sum_b t1[b], grad_gamma = sum_b t2[b] (ascending b),
 *                      T1[b, g] = sum_{ch in g} gamma[ch] * t1[b, ch], T2 likewise (ascending ch),
 *                      dx[i, ch] = rstd[b, g] * (gamma[ch] * dy[i, ch] - T1[b, g] / m - xhat[i, ch] * T2[b, g] / m).
 *                      gamma may be NULL (1); dx, grad_gamma and grad_beta may each be NULL (skipped).
 * Host-side argument errors (non-zero return, message in me_last_error, nothing launched): groups <= 0 or
 * c % groups != 0; a workspace smaller than me_gnorm_workspace_bytes(n, n_batch, c, groups); more than 3225 channels
 * (the 64 KiB of LDS of the partial kernels; fp32 / bf16 entry points only).  The _f64 entry points are the same formulae
 * in plain double (parameters and statistics double as well): the yardstick of gradcheck, not a hot path. */
int64_t me_gnorm_workspace_bytes(int64_t n, int32_t n_batch, int32_t c, int32_t groups);
int me_gnorm_stats(const void *x_dev, int32_t is_bf16, const int32_t *batch_row_dev, int64_t n, int32_t n_batch,
                   int32_t c, int32_t groups, float eps, float *mean_dev, float *rstd_dev, void *workspace_dev,
                   int64_t workspace_bytes, void *stream);
int me_gnorm_apply(const void *x_dev, int32_t is_bf16, const int32_t *batch_row_dev, int64_t n, int32_t n_batch,
                   int32_t c, int32_t groups, const float *mean_dev, const float *rstd_dev, const float *gamma_dev,
                   const float *beta_dev, void *y_dev, void *stream);
int me_gnorm_backward(const void *x_dev, const void *dy_dev, int32_t is_bf16, const int32_t *batch_row_dev, int64_t n,
                      int32_t n_batch, int32_t c, int32_t groups, const float *mean_dev, const float *rstd_dev,
                      const float *gamma_dev, void *dx_dev, float *grad_gamma_dev, float *grad_beta_dev,
                      void *workspace_dev, int64_t workspace_bytes, void *stream);
int me_gnorm_stats_f64(const double *x_dev, const int32_t *batch_row_dev, int64_t n, int32_t n_batch, int32_t c,
                       int32_t groups, double eps, double *mean_dev, double *rstd_dev, void *stream);
int me_gnorm_apply_f64(const double *x_dev, const int32_t *batch_row_dev, int64_t n, int32_t n_batch, int32_t c,
                       int32_t groups, const double *mean_dev, const double *rstd_dev, const double *gamma_dev,
                       const double *beta_dev, double *y_dev, void *stream);
int me_gnorm_backward_f64(const double *x_dev, const double *dy_dev, const int32_t *batch_row_dev, int64_t n,
                          int32_t n_batch, int32_t c, int32_t groups, const double *mean_dev, const double *rstd_dev,
                          const double *gamma_dev, double *dx_dev, double *grad_gamma_dev, double *grad_beta_dev,
                          void *workspace_dev, int64_t workspace_bytes, void *stream);

/* ---- conditional group normalisation (MinkowskiConditionalGroupNorm: AdaGN / FiLM; csrc/group_norm.hip, ABI 1.16) ----
 * Group normalisation whose affine map is modulated per instance and followed by an optional SiLU.  The statistics are
 * me_gnorm_stats' (mean / rstd [n_batch, groups]).  scale / shift: [n_batch, c] in the parameter type, row b for the
 * instance b of batch_row; act: 0 identity, 1 SiLU.
 *   ge[b, ch] = gamma[ch] * (1 + scale[b, ch]),  be[b, ch] = beta[ch] * (1 + scale[b, ch]) + shift[b, ch]
 *   me_gnorm_cond_apply:    v = xhat * ge[b, ch] + be[b, ch], y = act(v)      (SiLU: v * sigmoid(v), in fp32)
 *   me_gnorm_cond_backward: dv = dy * act'(v) with v recomputed from x; t1[b, ch] = sum_{i in b} dv, t2 = sum dv * xhat;
 *                           grad_shift = t1, grad_scale = gamma * t2 + beta * t1, grad_beta = sum_b (1 + scale) * t1,
 *                           grad_gamma = sum_b (1 + scale) * t2 (ascending b); T1[b, g] = sum_{ch in g} ge * t1, T2
 *                           likewise (ascending ch); dx = rstd * (ge * dv - T1 / m - xhat * T2 / m), m = n_b * cg.
 * gamma, beta, scale, shift (1 / 0 / 0 / 0) and dx and every gradient pointer (skipped) may be NULL; every requested word is
 * written, the grad_scale / grad_shift rows of an instance without rows with exactly 0.  No atomics on values, fixed
 * summation order.  ge / be live in the workspace (me_gnorm_cond_workspace_bytes >= me_gnorm_workspace_bytes), which the
 * apply needs too.  Host-side argument errors (nothing launched): act other than 0 / 1; groups <= 0 or c % groups != 0; a
 * short workspace; more than 3225 channels (fp32 / bf16 entry points).  The _f64 entry points: plain double, parameters,
 * scale / shift and statistics double. */
int64_t me_gnorm_cond_workspace_bytes(int64_t n, int32_t n_batch, int32_t c, int32_t groups);
int me_gnorm_cond_apply(const void *x_dev, int32_t is_bf16, const int32_t *batch_row_dev, int64_t n, int32_t n_batch,
                        int32_t c, int32_t groups, const float *mean_dev, const float *rstd_dev, const float *gamma_dev,
                        const float *beta_dev, const float *scale_dev, const float *shift_dev, int32_t act, void *y_dev,
                        void *workspace_dev, int64_t workspace_bytes, void *stream);
int me_gnorm_cond_backward(const void *x_dev, const void *dy_dev, int32_t is_bf16, const int32_t *batch_row_dev,
                           int64_t n, int32_t n_batch, int32_t c, int32_t groups, const float *mean_dev,
                           const float *rstd_dev, const float *gamma_dev, const float *beta_dev, const float *scale_dev,
                           const float *shift_dev, int32_t act, void *dx_dev, float *grad_gamma_dev, float *grad_beta_dev,
                           float *grad_scale_dev, float *grad_shift_dev, void *workspace_dev, int64_t workspace_bytes,
                           void *stream);
int me_gnorm_cond_apply_f64(const double *x_dev, const int32_t *batch_row_dev, int64_t n, int32_t n_batch, int32_t c,
                            int32_t groups, const double *mean_dev, const double *rstd_dev, const double *gamma_dev,
                            const double *beta_dev, const double *scale_dev, const double *shift_dev, int32_t act,
                            double *y_dev, void *stream);
int me_gnorm_cond_backward_f64(const double *x_dev, const double *dy_dev, const int32_t *batch_row_dev, int64_t n,
                               int32_t n_batch, int32_t c, int32_t groups, const double *mean_dev, const double *rstd_dev,
                               const double *gamma_dev, const double *beta_dev, const double *scale_dev,
                               const double *shift_dev, int32_t act, double *dx_dev, double *grad_gamma_dev,
                               double *grad_beta_dev, double *grad_scale_dev, double *grad_shift_dev, void *workspace_dev,
                               int64_t workspace_bytes, void *stream);

/* ---- per-instance multi-head attention (MinkowskiSelfAttention, MinkowskiFunctional.scaled_dot_product_attention;
 *      csrc/attention.hip, ABI 1.17) ----
 * q: [n_q, c] rows on map A; k, v: [n_kv, c] rows on map B; c = heads * d.  For query row i, head h and its instance b(i):
 *   s_ij = scale * <q[i, h, :], k[j, h, :]> over the rows j of B with b(j) = b(i)
 *   out[i, h, :] = sum_j softmax_j(s_ij) * v[j, h, :],   lse[i, h] = log sum_j exp(s_ij)   ([n_q, heads] fp32, contiguous)
 * A query whose instance has no row on B: a zero output row, lse = -inf, zero gradients.  The rows of instance b are
 * seg_rows[seg_ptr[b] .. seg_ptr[b + 1]) in ascending order (me_csr_from_coo of the origin rows of the map, n_batch rows);
 * keys are summed in that order.  Every operand carries a row stride in elements: >= c, a multiple of 16 bytes, last
 * dimension contiguous, base pointers 16-byte aligned (the column slices of one [n, 3 c] projection go in without copies).
 * fp32 / bf16 entry points: d in {32, 64, 128}, softmax and statistics in fp32, P and dS rounded to bf16 on bf16 rows.
 * me_attn_backward: dq / dk / dv may be NULL (not computed; the dK / dV launch is skipped when both are, the dQ launch when
 * dq is); the workspace (me_attn_workspace_bytes) holds delta[i, h] = <dout_i, out_i>.  No atomics, fixed summation order:
 * bitwise reproducible.  Host-side argument errors (nothing launched, reachable with NULL data pointers): c % heads != 0; a
 * head dimension other than 32 / 64 / 128; a stride below c or not a multiple of 16 bytes; a short workspace; a missing
 * table pointer.  The _f64 entry points: plain double, any head dimension, any stride >= c, lse double, no workspace. */
int64_t me_attn_workspace_bytes(int64_t n_q, int64_t n_kv, int32_t n_batch, int32_t heads);
int me_attn_forward(const void *q_dev, const void *k_dev, const void *v_dev, int32_t is_bf16, int64_t q_stride,
                    int64_t k_stride, int64_t v_stride, const int32_t *seg_ptr_q_dev, const int32_t *seg_rows_q_dev,
                    const int32_t *seg_ptr_kv_dev, const int32_t *seg_rows_kv_dev, int64_t n_q, int64_t n_kv,
                    int32_t n_batch, int32_t c, int32_t heads, float scale, void *out_dev, int64_t out_stride,
                    float *lse_dev, void *stream);
int me_attn_backward(const void *q_dev, const void *k_dev, const void *v_dev, const void *out_dev, const float *lse_dev,
                     const void *dout_dev, int32_t is_bf16, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                     int64_t out_stride, int64_t dout_stride, const int32_t *seg_ptr_q_dev, const int32_t *seg_rows_q_dev,
                     const int32_t *seg_ptr_kv_dev, const int32_t *seg_rows_kv_dev, int64_t n_q, int64_t n_kv,
                     int32_t n_batch, int32_t c, int32_t heads, float scale, void *dq_dev, int64_t dq_stride, void *dk_dev,
                     int64_t dk_stride, void *dv_dev, int64_t dv_stride, void *workspace_dev, int64_t workspace_bytes,
                     void *stream);
int me_attn_forward_f64(const double *q_dev, const double *k_dev, const double *v_dev, int64_t q_stride, int64_t k_stride,
                        int64_t v_stride, const int32_t *seg_ptr_q_dev, const int32_t *seg_rows_q_dev,
                        const int32_t *seg_ptr_kv_dev, const int32_t *seg_rows_kv_dev, int64_t n_q, int64_t n_kv,
                        int32_t n_batch, int32_t c, int32_t heads, double scale, double *out_dev, int64_t out_stride,
                        double *lse_dev, void *stream);
int me_attn_backward_f64(const double *q_dev, const double *k_dev, const double *v_dev, const double *out_dev,
                         const double *lse_dev, const double *dout_dev, int64_t q_stride, int64_t k_stride,
                         int64_t v_stride, int64_t out_stride, int64_t dout_stride, const int32_t *seg_ptr_q_dev,
                         const int32_t *seg_rows_q_dev, const int32_t *seg_ptr_kv_dev, const int32_t *seg_rows_kv_dev,
                         int64_t n_q, int64_t n_kv, int32_t n_batch, int32_t c, int32_t heads, double scale, double *dq_dev,
                         int64_t dq_stride, double *dk_dev, int64_t dk_stride, double *dv_dev, int64_t dv_stride,
                         void *stream);

/* ---- local attention over a kernel map (MinkowskiLocalSelfAttention, MinkowskiFunctional.local_attention;
 *      csrc/local_attention.hip, ABI 1.18) ----
 * q: [n_out, c] rows on the out map; k, v: [n_in, c] rows on the in map; c = heads * d.  nbr_out: int32 [volume, n_out],
 * the in row of offset k of out row i or -1; nbr_in: int32 [volume, n_in], its transpose (the out row that sees in row j
 * through offset k, or -1) — the dense tables of a pooling kernel map.  For out row i, head h and the offsets k in
 * ascending order with j = nbr_out[k][i] >= 0:
 *   s_ik = scale * <q[i, h, :], k[j, h, :]> + rel_pos_bias[h, k]      (rel_pos_bias: fp32 [heads, volume] or NULL = 0)
 *   out[i, h, :] = sum_k softmax_k(s_ik) v[j, h, :],   lse[i, h] = log sum_k exp(s_ik)   ([n_out, heads] fp32, contiguous)
 * lse_lo ([n_out, heads] fp32 or NULL): the residual (m + log l) - lse of the fp32 rounding of lse; the backward pass
 * subtracts it too, so that the weights it recomputes add up to 1 like the forward ones when |lse| is in the hundreds.
 * A row without a neighbour: a zero output row, lse = -inf, zero gradients.  A hole is never read as a value.  Every
 * operand carries a row stride in elements: >= c, a multiple of 16 bytes, last dimension contiguous, base pointers 16-byte
 * aligned (the column slices of one [n, 3 c] projection go in without copies).  fp32 / bf16 entry points: d a power of two
 * from 8 to 128; scores, softmax and sums in fp32, one rounding at the store.  me_local_attn_backward: dq / dk / dv /
 * grad_rel_pos_bias (fp32 [heads, volume]) may be NULL (not computed; the dK / dV launch is skipped when both are, the
 * walk of the dQ launch when neither dq nor the bias gradient is wanted); the workspace
 * (me_local_attn_workspace_bytes; with_bias: the bias gradient is wanted) holds delta[i, h] = <dout_i, out_i> and the
 * per-workgroup sums of the bias gradient.  No atomics, fixed summation order: bitwise reproducible.  Host-side argument
 * errors (nothing launched, reachable with NULL data pointers): c % heads != 0; a head dimension outside the rule; a stride
 * below c or not a multiple of 16 bytes; a short workspace; a missing table pointer; volume < 1 or > 2^20; out rows
 * without in rows.  The _f64 entry points: plain double, any head dimension, any stride >= c, lse, bias and its gradient
 * double, no workspace. */
int64_t me_local_attn_workspace_bytes(int64_t n_out, int32_t heads, int64_t volume, int32_t with_bias);
int me_local_attn_forward(const void *q_dev, const void *k_dev, const void *v_dev, int32_t is_bf16, int64_t q_stride,
                          int64_t k_stride, int64_t v_stride, const int32_t *nbr_out_dev, int64_t n_out, int64_t n_in,
                          int64_t volume, int32_t c, int32_t heads, float scale, const float *rel_pos_bias_dev,
                          void *out_dev, int64_t out_stride, float *lse_dev, float *lse_lo_dev, void *stream);
int me_local_attn_backward(const void *q_dev, const void *k_dev, const void *v_dev, const void *out_dev,
                           const float *lse_dev, const float *lse_lo_dev, const void *dout_dev, int32_t is_bf16, int64_t q_stride, int64_t k_stride,
                           int64_t v_stride, int64_t out_stride, int64_t dout_stride, const int32_t *nbr_out_dev,
                           const int32_t *nbr_in_dev, int64_t n_out, int64_t n_in, int64_t volume, int32_t c,
                           int32_t heads, float scale, const float *rel_pos_bias_dev, void *dq_dev, int64_t dq_stride,
                           void *dk_dev, int64_t dk_stride, void *dv_dev, int64_t dv_stride,
                           float *grad_rel_pos_bias_dev, void *workspace_dev, int64_t workspace_bytes, void *stream);
int me_local_attn_forward_f64(const double *q_dev, const double *k_dev, const double *v_dev, int64_t q_stride,
                              int64_t k_stride, int64_t v_stride, const int32_t *nbr_out_dev, int64_t n_out, int64_t n_in,
                              int64_t volume, int32_t c, int32_t heads, double scale, const double *rel_pos_bias_dev,
                              double *out_dev, int64_t out_stride, double *lse_dev, void *stream);
int me_local_attn_backward_f64(const double *q_dev, const double *k_dev, const double *v_dev, const double *out_dev,
                               const double *lse_dev, const double *dout_dev, int64_t q_stride, int64_t k_stride,
                               int64_t v_stride, int64_t out_stride, int64_t dout_stride, const int32_t *nbr_out_dev,
                               const int32_t *nbr_in_dev, int64_t n_out, int64_t n_in, int64_t volume, int32_t c,
                               int32_t heads, double scale, const double *rel_pos_bias_dev, double *dq_dev,
                               int64_t dq_stride, double *dk_dev, int64_t dk_stride, double *dv_dev, int64_t dv_stride,
                               double *grad_rel_pos_bias_dev, void *stream);

/* ---- serialized patch attention (MinkowskiSerializedSelfAttention, MinkowskiFunctional.serialized_attention;
 *      csrc/serial_attention.hip and csrc/attention.hip, ABI 1.19) ----
 * The rows of every instance are ordered along a space-filling curve, cut into patches of at most patch_size rows, and
 * the kernels of me_attn_forward / me_attn_backward attend inside every patch: a patch is a segment of their row lists.
 *
 * me_coords_serial_keys: keys[i] = ((uint32) coords[i, 0] << D * depth) | code(x), D = ncol - 1,
 *   x_a = (coords[i, 1 + a] - bbox_min[a]) / tensor_stride[a] (exact on a map of that stride; x_a < 2^depth, so depth is
 *   the bit count of the largest x_a of the map; tensor_stride and bbox_min: D host ints; the difference is taken in
 *   uint32, so it is exact for every extent of an int32 map, 2^31 and more included).  order:
 *     0  z              bit l of axis a at code bit l * D + (D - 1 - a): axis 0 is the most significant of a level
 *     2  hilbert        Skilling's AxesToTranspose (Programming the Hilbert curve, 2004) on x with depth bits, the
 *                       transposed axes interleaved by the rule of z
 *     1, 3  z_trans, hilbert_trans: the same codes with the spatial axes 0 and 1 exchanged beforehand (D >= 2)
 *   Host-side error, nothing launched: D * depth > 63.
 *
 * me_attn_patch_lists: keys, the library's stable radix sort over the significant key bytes, and for an instance of n_b
 * rows m_b = ceil(n_b / patch_size) patches, the row of serial rank r going to patch floor(r * m_b / n_b) (64-bit): sizes
 * differ by at most one, none exceeds patch_size, no row is shared.  Outputs, with S = ceil(n / patch_size) + n_batch
 * segments (an upper bound of the patch count; surplus segments are empty):
 *   row_patch int32 [n]       the global patch of every row: patches are numbered by ascending batch index, then rank
 *   seg_ptr   int32 [S + 1], seg_rows int32 [n]   me_csr_from_coo of row_patch: rows ascending inside a patch
 *   blk_tab   int32 [2 * (ceil(n / 64) + S)]      for every 64-row block of every non-empty segment, in segment order,
 *                                                (segment, first row in the segment); unused entries hold segment -1
 * n_batch: the number of instances (at least the number of distinct batch indices); batch_max: the largest batch index
 * (batch indices are >= 0).  No synchronisation, no read-back.  Host-side errors, nothing launched: patch_size < 1, an
 * unknown order, D * depth + bits(max(batch_max, n_batch)) > 63, a short workspace.
 *
 * me_attn_forward_tab / me_attn_backward_tab (and _f64): me_attn_forward / me_attn_backward with n_batch read as the
 * number of segments of any row lists, plus one optional block table per side (NULL: the workgroups walk seg_ptr, which
 * is what me_attn_forward / me_attn_backward do).  A table belongs to its row lists and has ceil(n_side / 64) + n_batch
 * pairs in the layout above; the q-side table is read by the forward and the dQ kernels, the kv-side table by the dK / dV
 * kernel, and the float64 twins accept and ignore both.  Lists and table are generic: any partition of the rows into
 * segments (patches here, windows elsewhere) is attended the same way.  Same arguments, errors and results otherwise. */
int me_coords_serial_keys(const int32_t *coords_dev, int64_t n, int32_t ncol, const int32_t *tensor_stride,
                          const int32_t *bbox_min, int32_t depth, int32_t order, uint64_t *keys_dev, void *stream);
int64_t me_attn_patch_lists_workspace_bytes(int64_t n, int32_t n_batch, int64_t patch_size);
int me_attn_patch_lists(const int32_t *coords_dev, int64_t n, int32_t ncol, const int32_t *tensor_stride,
                        const int32_t *bbox_min, int32_t depth, int32_t batch_max, int32_t order, int32_t n_batch,
                        int64_t patch_size, int32_t *seg_ptr_dev, int32_t *seg_rows_dev, int32_t *blk_tab_dev,
                        int32_t *row_patch_dev, void *workspace_dev, int64_t workspace_bytes, void *stream);
int me_attn_forward_tab(const void *q_dev, const void *k_dev, const void *v_dev, int32_t is_bf16, int64_t q_stride,
                        int64_t k_stride, int64_t v_stride, const int32_t *seg_ptr_q_dev, const int32_t *seg_rows_q_dev,
                        const int32_t *seg_ptr_kv_dev, const int32_t *seg_rows_kv_dev, const int32_t *blk_tab_q_dev,
                        const int32_t *blk_tab_kv_dev, int64_t n_q, int64_t n_kv, int32_t n_batch, int32_t c,
                        int32_t heads, float scale, void *out_dev, int64_t out_stride, float *lse_dev, void *stream);
int me_attn_backward_tab(const void *q_dev, const void *k_dev, const void *v_dev, const void *out_dev,
                         const float *lse_dev, const void *dout_dev, int32_t is_bf16, int64_t q_stride, int64_t k_stride,
                         int64_t v_stride, int64_t out_stride, int64_t dout_stride, const int32_t *seg_ptr_q_dev,
                         const int32_t *seg_rows_q_dev, const int32_t *seg_ptr_kv_dev, const int32_t *seg_rows_kv_dev,
                         const int32_t *blk_tab_q_dev, const int32_t *blk_tab_kv_dev, int64_t n_q, int64_t n_kv,
                         int32_t n_batch, int32_t c, int32_t heads, float scale, void *dq_dev, int64_t dq_stride,
                         void *dk_dev, int64_t dk_stride, void *dv_dev, int64_t dv_stride, void *workspace_dev,
                         int64_t workspace_bytes, void *stream);
int me_attn_forward_tab_f64(const double *q_dev, const double *k_dev, const double *v_dev, int64_t q_stride,
                            int64_t k_stride, int64_t v_stride, const int32_t *seg_ptr_q_dev,
                            const int32_t *seg_rows_q_dev, const int32_t *seg_ptr_kv_dev, const int32_t *seg_rows_kv_dev,
                            const int32_t *blk_tab_q_dev, const int32_t *blk_tab_kv_dev, int64_t n_q, int64_t n_kv,
                            int32_t n_batch, int32_t c, int32_t heads, double scale, double *out_dev, int64_t out_stride,
                            double *lse_dev, void *stream);
int me_attn_backward_tab_f64(const double *q_dev, const double *k_dev, const double *v_dev, const double *out_dev,
                             const double *lse_dev, const double *dout_dev, int64_t q_stride, int64_t k_stride,
                             int64_t v_stride, int64_t out_stride, int64_t dout_stride, const int32_t *seg_ptr_q_dev,
                             const int32_t *seg_rows_q_dev, const int32_t *seg_ptr_kv_dev,
                             const int32_t *seg_rows_kv_dev, const int32_t *blk_tab_q_dev, const int32_t *blk_tab_kv_dev,
                             int64_t n_q, int64_t n_kv, int32_t n_batch, int32_t c, int32_t heads, double scale,
                             double *dq_dev, int64_t dq_stride, double *dk_dev, int64_t dk_stride, double *dv_dev,
                             int64_t dv_stride, void *stream);

/* ---- shifted-window attention (MinkowskiWindowSelfAttention, MinkowskiFunctional.window_attention;
 *      csrc/serial_attention.hip, ABI 1.21) ----
 * Space is cut into axis-aligned boxes of window_size[a] cells of the tensor stride per spatial axis a < D = ncol - 1, on a
 * grid anchored at the origin of the coordinate system and moved by shift[a] cells; the kernels of me_attn_forward_tab /
 * me_attn_backward_tab attend inside every box: a window is a segment of their row lists.  The window of the row
 * (b, c_0 .. c_{D-1}) is (b, cell_0 .. cell_{D-1}) with
 *   cell_a = floor((floor(c_a / t_a) + s_a) / w_a),   s_a = shift[a] modulo w_a in [0, w_a)
 * both floors towards -inf, so negative coordinates are legal and shift and shift + window_size give the same partition.
 * Nothing is padded, there is no cyclic wrap and no mask.
 *
 * me_attn_window_ids: row_window int32 [n], the window of every row, the windows numbered 0 .. W - 1 in ascending
 *   lexicographic order of (b, cell_0 .. cell_{D-1}); *n_windows_dev (int32, device memory) = W.  tensor_stride,
 *   window_size, shift, bbox_min, bbox_max: n_axes = D host ints each; bbox_min / bbox_max: the smallest and the largest
 *   coordinate of every spatial axis (any box that holds every row will do); batch_min / batch_max: the smallest and the
 *   largest batch index.  A key packs b above the fields of cell_a - cell_lo_a (cell_lo_a the cell of bbox_min[a], a field
 *   the bit count of the largest difference in the box), the library's stable radix sort orders the significant key bytes,
 *   and the rank of a row's key among the distinct keys is its window.  Difference and quotient are taken in 64 bits: exact
 *   for every int32 coordinate and every extent, 2^31 and more included.  No synchronisation, no read-back.
 *   Workspace: me_attn_window_ids_workspace_bytes(n).  Host-side errors, nothing launched: a window size below 1,
 *   n_axes != D, window_size[a] * tensor_stride[a] >= 2^31, a negative batch index, the cell bits of all axes + the bits of
 *   batch_max > 63, a short workspace.
 *
 * me_attn_segment_lists: the row lists and the block table of ANY segment id per row (row_segment int32 [n], every value
 *   in [0, n_seg)), in the layout of me_attn_patch_lists:
 *   seg_ptr   int32 [n_seg + 1], seg_rows int32 [n]   me_csr_from_coo of row_segment: rows ascending inside a segment
 *   blk_tab   int32 [2 * (ceil(n / 64) + n_seg)]      for every 64-row block of every non-empty segment, in segment order,
 *                                                    (segment, first row in the segment); unused entries hold segment -1
 *   No synchronisation, no read-back.  Workspace: me_attn_segment_lists_workspace_bytes(n, n_seg).  Host-side errors,
 *   nothing launched: n or n_seg beyond int32, rows with n_seg = 0, a short workspace, a null output.
 * A caller that wants no surplus workgroups reads *n_windows_dev back once (4 bytes) and passes it as n_seg; without the
 * read-back min(n, cells in the box) is the only bound the host knows. */
int64_t me_attn_window_ids_workspace_bytes(int64_t n);
int me_attn_window_ids(const int32_t *coords_dev, int64_t n, int32_t ncol, const int32_t *tensor_stride,
                       const int32_t *window_size, const int32_t *shift, int32_t n_axes, const int32_t *bbox_min,
                       const int32_t *bbox_max, int32_t batch_min, int32_t batch_max, int32_t *row_window_dev,
                       int32_t *n_windows_dev, void *workspace_dev, int64_t workspace_bytes, void *stream);
int64_t me_attn_segment_lists_workspace_bytes(int64_t n, int64_t n_seg);
int me_attn_segment_lists(const int32_t *row_segment_dev, int64_t n, int64_t n_seg, int32_t *seg_ptr_dev,
                          int32_t *seg_rows_dev, int32_t *blk_tab_dev, void *workspace_dev, int64_t workspace_bytes,
                          void *stream);

/* ---- rotary position embedding from voxel coordinates (MinkowskiRotaryEmbedding, MinkowskiFunctional.rotary_embedding,
 *      the rope= argument of the self-attention modules; csrc/rope.hip, ABI 1.22) ----
 * x is [n, heads * d] on a coordinate map with D = ncol - 1 spatial axes.  d is even and P = d / 2 >= D.  Pairs are
 * interleaved: pair p of a head is the channels (2p, 2p + 1) of that head; every head takes the same angles.
 *   m = P / D (integer division) frequencies per axis; pair p < D * m belongs to axis a = p / m and frequency j = p % m;
 *   the P - D * m trailing pairs pass through unchanged (cos 1, sin 0).
 *   omega_j = base^(-j / m), computed once per call on the host in double (pow), inside the library.
 *   theta   = ((double)c_a / (double)u_a) * omega_j, evaluated in that order; u_a >= 1 is the unit of axis a (the host
 *             layers pass the tensor stride of the map by default; no floor is taken, queries and keys on maps of
 *             different strides take one common unit).
 *   y[2p]     = x[2p] cos(theta) - s x[2p + 1] sin(theta)
 *   y[2p + 1] = s x[2p] sin(theta) + x[2p + 1] cos(theta)        s = sign = +1 forward, -1 backward
 * The rotation is orthogonal: the backward pass of the operator is the operator with sign = -1 applied to the gradient of
 * the output.  After it <y_i, y_j> of two rows depends on c_i - c_j only.
 *
 * me_rope_table: table[n][P][2] = (cos theta, sin theta), float (table_f64 = 0; for fp32 and bf16 rows) or double
 *   (table_f64 != 0; for float64 rows), 16-byte aligned.  Angle, range reduction and sin / cos are in double, the values
 *   rounded once.  unit: D host ints.  One launch, no synchronisation, no read-back, no workspace.
 *   Host-side errors, nothing launched: ncol outside [2, 8], d odd or below 2, d / 2 < D, d / 2 > ME_ROPE_MAX_PAIRS (the
 *   angular frequencies travel in the kernel arguments), base not finite or <= 0, a unit below 1, n >= 2^31, a null coords
 *   or table with n > 0, a table that is not 16-byte aligned.  n = 0 succeeds without a launch.
 *
 * me_rope_apply: y[i] = rotation of x[i] by sign * theta for the n rows; x and y are rows of heads * d elements of `dtype`
 *   with the row strides x_stride, y_stride >= heads * d (in elements), so a column view of a wider matrix is taken as it
 *   is; y may be x itself (a thread reads its piece before it writes it), any other overlap is undefined.  table: the
 *   me_rope_table of the same map, d, base and unit, float for ME_ROPE_F32 / ME_ROPE_BF16 rows, double for ME_ROPE_F64.
 *   bf16 rows are widened to fp32, rotated there and rounded once: the result equals the ME_ROPE_F32 result of the
 *   widened rows, rounded to bf16, bit for bit.  Rows are moved in 16-byte pieces (8 bf16, 4 fp32, 2 double) when x, y
 *   are 16-byte aligned and both strides and d are multiples of the piece; pair by pair otherwise, with the same bits.
 *   One launch (at most 2048 workgroups, grid-stride), no LDS, no atomics, no synchronisation, no read-back, bitwise
 *   reproducible.
 *   Host-side errors, nothing launched: d odd or below 2, d / 2 > ME_ROPE_MAX_PAIRS, heads < 1, heads * d or n >= 2^31,
 *   sign not +1 / -1, an unknown dtype, a row stride below heads * d, a null x, y or table with n > 0, x or y not aligned to
 *   an element or a table not aligned to 16 bytes.  n = 0 succeeds without a launch. */
#define ME_ROPE_MAX_PAIRS 128 /* P = d / 2 <= 128: heads of up to 256 channels */
#define ME_ROPE_F32 0
#define ME_ROPE_BF16 1
#define ME_ROPE_F64 2
int me_rope_table(const int32_t *coords_dev, int64_t n, int32_t ncol, const int32_t *unit, int32_t d, double base,
                  int32_t table_f64, void *table_dev, void *stream);
int me_rope_apply(const void *x_dev, int64_t x_stride, void *y_dev, int64_t y_stride, int64_t n, int32_t heads, int32_t d,
                  const void *table_dev, int32_t sign, int32_t dtype, void *stream);

/* ---- cross-attention to a dense context (MinkowskiCrossAttention, MinkowskiFunctional.cross_attention;
 *      csrc/attention.hip, ABI 1.20) ----
 * The queries are the rows of a coordinate map, the keys / values the rows of a dense context [n_batch, tokens, c]: one
 * more partition of rows into segments for me_attn_forward_tab and the dQ kernel of the backward pass.
 *
 * me_attn_context_lists: segment b holds the rows b * tokens + t for t < len_b, len_b = tokens when lengths_dev is NULL,
 *   else lengths_dev[b] clamped on the device to [0, tokens].  One launch, no read-back.  seg_ptr int32 [n_batch + 1];
 *   seg_rows int32 [n_batch * tokens], written up to seg_ptr[n_batch]; blk_tab int32 [2 * (ceil(n_batch * tokens / 64) +
 *   n_batch)] in the layout of me_attn_patch_lists (unused entries hold segment -1).  A thread sums the lengths before its
 *   instance itself (O(n_batch) loads).  Host-side errors, nothing launched: tokens < 1, n_batch < 0, n_batch * tokens
 *   >= 2^31, a null output.
 *
 * me_attn_backward_split: me_attn_backward_tab whose dK / dV pass is cut into kv_splits query slices.  The dK / dV kernel
 *   of me_attn_backward is key-stationary: (ceil(n_kv / 64) + n_batch) * heads workgroups, each walking every query of its
 *   instance — a few dozen workgroups under tens of thousands of queries when the keys are a short context.  With
 *   kv_splits = S > 1 slice s of an instance of nblk = ceil(len_q / 32) query blocks walks the blocks
 *   [floor(s nblk / S), floor((s + 1) nblk / S)) (a slice may be empty) and writes unscaled fp32 partials of the wanted
 *   gradients to the workspace [S][n_kv][c]; a reduce kernel sums them in ascending s, scales dK, rounds once and writes
 *   every gradient row once — zeros into a key row that no list holds.  No atomics: bitwise reproducible for a given S.
 *   kv_splits = 1 runs the launches of me_attn_backward_tab, bit for bit (which leave a key row on no list unwritten).
 *   Host-side errors, nothing launched: kv_splits < 1 or > ME_ATTN_MAX_KV_SPLITS, a workspace below
 *   me_attn_split_workspace_bytes, and the errors of me_attn_backward_tab.  The float64 twin accepts and ignores
 *   kv_splits and the tables; it too leaves a key row on no list unwritten.
 * me_attn_split_workspace_bytes: delta [n_q, heads] fp32, one int32 mark per key row, and the two partial images of
 *   kv_splits * n_kv * c fp32 each (every part rounded up to 256 bytes); for every kv_splits >= 1.
 * me_attn_kv_splits: the policy of the operators, a pure function of the shape (host only).  With wgs = (ceil(n_kv / 64) +
 *   n_batch) * heads workgroups in the key-stationary grid, S = floor(512 / wgs): 512 workgroups are one round on the
 *   chip (two on each of 256 CUs at one wave per SIMD), so the slices add no second round.  S = 1 as soon as wgs > 256 —
 *   every self-attention shape with n_kv = n_q > 64 * 256 / heads.  Bounded by ME_ATTN_MAX_KV_SPLITS (32), by at least
 *   256 queries of an average instance per slice (S <= n_q / n_batch / 256), and by 64 MiB of partial images
 *   (2 * S * n_kv * c * 4 bytes); at least 1.  DESIGN.md 8.14 has the measurement behind the bounds. */
#define ME_ATTN_MAX_KV_SPLITS 32
int me_attn_context_lists(int32_t n_batch, int32_t tokens, const int32_t *lengths_dev, int32_t *seg_ptr_dev,
                          int32_t *seg_rows_dev, int32_t *blk_tab_dev, void *stream);
int32_t me_attn_kv_splits(int64_t n_q, int64_t n_kv, int32_t n_batch, int32_t c, int32_t heads);
int64_t me_attn_split_workspace_bytes(int64_t n_q, int64_t n_kv, int32_t n_batch, int32_t c, int32_t heads,
                                      int32_t kv_splits);
int me_attn_backward_split(const void *q_dev, const void *k_dev, const void *v_dev, const void *out_dev,
                           const float *lse_dev, const void *dout_dev, int32_t is_bf16, int64_t q_stride,
                           int64_t k_stride, int64_t v_stride, int64_t out_stride, int64_t dout_stride,
                           const int32_t *seg_ptr_q_dev, const int32_t *seg_rows_q_dev, const int32_t *seg_ptr_kv_dev,
                           const int32_t *seg_rows_kv_dev, const int32_t *blk_tab_q_dev, const int32_t *blk_tab_kv_dev,
                           int64_t n_q, int64_t n_kv, int32_t n_batch, int32_t c, int32_t heads, float scale,
                           void *dq_dev, int64_t dq_stride, void *dk_dev, int64_t dk_stride, void *dv_dev,
                           int64_t dv_stride, void *workspace_dev, int64_t workspace_bytes, int32_t kv_splits,
                           void *stream);
int me_attn_backward_split_f64(const double *q_dev, const double *k_dev, const double *v_dev, const double *out_dev,
                               const double *lse_dev, const double *dout_dev, int64_t q_stride, int64_t k_stride,
                               int64_t v_stride, int64_t out_stride, int64_t dout_stride, const int32_t *seg_ptr_q_dev,
                               const int32_t *seg_rows_q_dev, const int32_t *seg_ptr_kv_dev,
                               const int32_t *seg_rows_kv_dev, const int32_t *blk_tab_q_dev,
                               const int32_t *blk_tab_kv_dev, int64_t n_q, int64_t n_kv, int32_t n_batch, int32_t c,
                               int32_t heads, double scale, double *dq_dev, int64_t dq_stride, double *dk_dev,
                               int64_t dk_stride, double *dv_dev, int64_t dv_stride, int32_t kv_splits, void *stream);

/* ---- dense <-> sparse conversion (SparseTensor.dense, ME.to_sparse, ME.to_sparse_all, ME.dense_coordinates:
 *      MinkowskiEngine/MinkowskiSparseTensor.py:460-557 and MinkowskiOps.py:246-348, torch indexing there;
 *      csrc/dense.hip, ABI 1.10) ----
 * Feature rows [n, c] row-major <-> a strided box [outer, c, inner].  A cell is (o, i), its linear index o * inner + i =
 * its linear index over shape = (B, X1, .., XD), wherever the channel axis sits in the layout (outer = B, inner = X1*..*XD
 * for BCX..X; outer = B*X1*..*XD, inner = 1 for channels-last).  Values move as raw words of elem_bytes = 2 (bf16), 4
 * (fp32) or 8 (float64): copies, no arithmetic, no atomics, bitwise reproducible.  min_coord / divisor / shape are HOST
 * arrays of D / D / D+1 values.
 *   me_dense_cell_index:  cell[r] = linear index of (b, floor((x_k - min_coord_k) / divisor_k)) in `shape`, or -1 — and
 *                         *flag_dev = 1 (0 otherwise) — when row r lies outside the box on EITHER side.  No movers ever
 *                         write such a row.  min_coord / divisor NULL: 0 / 1.
 *   me_dense_grid:        grid[cell] = row of the cell, -1 = empty (int32 [n_cells]); unique coordinates: race-free.
 *   me_dense_rows_to_box: EVERY element of the box is written exactly once, zeros included.  ME_DENSE_CELL_STATIONARY:
 *                         tiles of 64 consecutive cells gather their rows (contiguous c-vectors) through the grid,
 *                         transpose through LDS and store coalesced along `inner` (128-bit stores when inner % 4 == 0 and
 *                         the box is 16-byte aligned); needs grid_dev.  ME_DENSE_ROW_STATIONARY: zero fill, then one wave per
 *                         row scatters its elements `inner` apart; needs cell_dev.  policy 0: cell-stationary when the grid
 *                         is given.  cell_dev == grid_dev == NULL: identity (row r is cell r, n == outer * inner).
 *   me_dense_box_to_rows: rows[r] = the c elements of cell[r]; the same two shapes backwards (cell-stationary reads the box
 *                         coalesced and pays for empty cells; it writes only rows the grid names; row-stationary writes
 *                         zeros into a row whose cell is -1).
 *   me_dense_policy:      host only; the cheaper shape for n rows in n_cells cells (to_box: 1 rows -> box, 0 box -> rows):
 *                         bytes moved, weighted by the measured rates of the two shapes (csrc/dense.hip).
 *   me_dense_occupied_count (SYNC) / me_dense_occupied_fill: cells with a channel that is not +-0 (= `abs(x).sum(ch) != 0`,
 *                         a NaN keeps its cell), in ASCENDING cell order (torch.where's order): count first, then, into
 *                         buffers of that many rows, coords [n, D+1] (batch first) and cell [n].  The workspace carries the
 *                         wave masks from count to fill.  Fewer than 2^31 cells.
 *   me_dense_all_coords:  coords [n_cells, D+1] of every cell in cell order (ME.dense_coordinates on the device). */
#define ME_DENSE_ROW_STATIONARY 1
#define ME_DENSE_CELL_STATIONARY 2
int me_dense_policy(int64_t n, int64_t n_cells, int32_t c, int32_t elem_bytes, int32_t to_box);
int me_dense_cell_index(const int32_t *coords_dev, int64_t n, int32_t ncol, const int32_t *min_coord,
                        const int32_t *divisor, const int64_t *shape, int64_t *cell_dev, int32_t *flag_dev, void *stream);
int me_dense_grid(const int64_t *cell_dev, int64_t n, int64_t n_cells, int32_t *grid_dev, void *stream);
int me_dense_rows_to_box(const void *rows_dev, int32_t elem_bytes, const int64_t *cell_dev, const int32_t *grid_dev,
                         int64_t n, int64_t outer, int32_t c, int64_t inner, void *box_dev, int32_t policy, void *stream);
int me_dense_box_to_rows(const void *box_dev, int32_t elem_bytes, const int64_t *cell_dev, const int32_t *grid_dev,
                         int64_t n, int64_t outer, int32_t c, int64_t inner, void *rows_dev, int32_t policy, void *stream);
int64_t me_dense_occupied_workspace_bytes(int64_t n_cells);
int me_dense_occupied_count(const void *box_dev, int32_t elem_bytes, int64_t outer, int32_t c, int64_t inner,
                            void *workspace_dev, int64_t workspace_bytes, int64_t *n_occupied, void *stream);
int me_dense_occupied_fill(const void *workspace_dev, int64_t workspace_bytes, int32_t ncol, const int64_t *shape,
                           int32_t *coords_dev, int64_t *cell_dev, void *stream);
int me_dense_all_coords(int32_t ncol, const int64_t *shape, int32_t *coords_dev, void *stream);

/* Plain VALU + atomics versions on the pair lists (debug cross-check only; never the default).
 * out / grad_in / grad_w must be zero-filled by the caller. */
int me_conv_forward_naive_f32(const float *in_feat_dev, int32_t c_in, const float *w_dev, int32_t c_out,
                              const int32_t *in_pairs_dev, const int32_t *out_pairs_dev,
                              const int64_t *k_offsets_dev, int64_t volume, int64_t n_pairs,
                              float *out_feat_dev, void *stream);
int me_conv_backward_naive_f32(const float *in_feat_dev, int32_t c_in, const float *grad_out_dev,
                               int32_t c_out, const float *w_dev, const int32_t *in_pairs_dev,
                               const int32_t *out_pairs_dev, const int64_t *k_offsets_dev,
                               int64_t volume, int64_t n_pairs, float *grad_in_dev,
                               float *grad_w_dev, void *stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* ME_AMD_H */
