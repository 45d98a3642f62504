// tr_kernels.h -- launchers of the HIP kernels (tr_kernels.hip).  Each returns 0 or a
// hipError_t value; none synchronizes, allocates or copies, so a caller may capture them.
#pragma once

#include <hip/hip_runtime_api.h>
#include <stddef.h>

#include "tr_aa.h"
#include "tr_accumulate.h"
#include "tr_ao.h"
#include "tr_composite.h"
#include "tr_convolve.h"
#include "tr_rank.h"
#include "tr_bilateral.h"
#include "tr_dof.h"
#include "tr_bloom.h"
#include "tr_grade.h"
#include "tr_layer.h"
#include "tr_ramp.h"
#include "tr_lines.h"
#include "tr_distance.h"
#include "tr_morph.h"
#include "tr_outline.h"
#include "tr_pack.h"
#include "tr_projector.h"
#include "tr_relight.h"
#include "tr_resize.h"
#include "tr_shadow_merge.h"
#include "tr_skin.h"
#include "tr_stats.h"
#include "tr_warp.h"
#include "tr_yuv.h"
#include "tr_types.h"

namespace tr {

// `start` / `done` (may be null) are attached to the kernel's own dispatch packet: `done` is
// signalled by the kernel's completion without a separate event packet, and the pair brackets
// exactly the kernel's execution when both are timing events.
//
// `group` (a table of n_frames argument structs in DEVICE memory; null = an ordinary launch) makes a launch a
// FUSED one over a group of frames (tr_scene_render_frames): the workgroups of frame f take entry f of the
// table; `a` (and `tile_count` / `order`) then only describe what the frames have in common -- mesh size,
// tile grid, record layout, bin capacity -- to the launcher.  launch_order reads each frame's counters and
// work lists from the TILE kernel's table (TileArgs::tile_count / order / list_len).
// Vertex stage: every polygon's record into a.recs, its tiles' counters bumped.
// `hurry`: nothing else is on the GPU and the caller's tile kernel waits for the chain (shapes for latency, not for
// running beside a tile kernel).  `xform`: a frame of the launch draws a transform table (DevMesh::inst_xform) -- the
// kernel with that branch; false: the kernel without it, which must then not meet such a table.
int launch_setup(int vs_kind, const SetupArgs &a, const SetupArgs *group, uint32_t n_frames, bool xform, bool hurry, hipStream_t st,
                 hipEvent_t start, hipEvent_t done);
// The frame's lit texel image (k_lit: the normal-map / specular closure once per texel); a.lit, a.texel_set etc. say where.
int launch_lit(int fs, const SetupArgs &a, const SetupArgs *group, uint32_t n_frames, hipStream_t st, hipEvent_t start, hipEvent_t done);
// Builds the tile kernel's work lists from the counters k_setup filled (same stream, after it) and gives every tile
// its range of the pool.  `one`: the pass's arguments (a per-frame launch); `group`: the fused launch's table.
int launch_order(const TileArgs &one, uint32_t n_tiles, const TileArgs *group, uint32_t n_frames, hipStream_t st, hipEvent_t start,
                 hipEvent_t done);
// Copies the records into the tiles' ranges, with each (polygon, tile) pair's coverage masks (same stream, after
// launch_order); counts the counters back down to zero.
int launch_bin(const SetupArgs &a, const SetupArgs *group, uint32_t n_frames, bool hurry, hipStream_t st, hipEvent_t start,
               hipEvent_t done);
// tile_waves: 4, 8 or 16 wavefronts per tile workgroup (see tr_types.h); shared != 0: the waves share the
// tile's bin and resolve through atomic keys instead of each owning a column of the tile (k_tile's
// SHARED parameter; falls back to columns when n_polygons or a.bin_cap exceed the key's fields).
// units_per_frame: workgroups per frame when the caller knows the pass's list lengths (tr_plan.h, group_grid_units;
// 0 = one per tile, which always suffices).
int launch_tile(int fs_kind, const TileArgs &a, int tile_waves, int shared, uint32_t n_polygons, const TileArgs *group,
                uint32_t n_frames, hipStream_t st, hipEvent_t start, hipEvent_t done, uint32_t units_per_frame = 0,
                bool fused_single = false);
// Does that launch run the interior form of its kernel -- compiled for frames made of whole tiles only (k_tile, INTERIOR:
// no per-pixel frame or band tests)?  The same arguments as launch_tile's; `fused`: a fused launch (group != null) or a
// fused_single one.  (TR_INTERIOR=0 in the environment: never.)
bool tile_launch_is_interior(int fs_kind, const TileArgs &a, int tile_waves, int shared, uint32_t n_polygons, bool fused);
int launch_materialize_depth(float *zbuf, uint32_t *zclean, const DevFrame &frame, hipStream_t st);
// The band's tiles of frame buffer `fb` into the page-locked host buffer `host` (device address of it), skipping the
// tiles that are zeros on both sides (fb_clean: the target's colour-clean flags; host_clean: the host buffer's own)
int launch_read_back(const uint8_t *fb, uint8_t *host, const uint32_t *fb_clean, uint32_t *host_clean, const DevFrame &frame,
                     hipStream_t st);
// The band's tiles of `fb` into a peer GPU's copy of the frame, skipping the tiles that are zeros on both sides
// (k_push_tiles; remote_clean: this rank's record of the peer's copy; poisoned: the exchange's error word).
int launch_push_tiles(const uint8_t *fb, uint8_t *peer, const uint32_t *fb_clean, uint32_t *remote_clean, const DevFrame &frame,
                      const uint32_t *poisoned, unsigned long long *bytes, hipStream_t st);
// The band's frame box-filtered by `factor` (2, 4, 8; width, height and the band's rows are multiples of it) into
// `out`, a frame of width / factor x height / factor pixels (device memory or the device address of mapped host
// memory): k_resolve.  fb_clean: the target's colour-clean flags (tiles not read, stored as zeros) or null.
int launch_resolve(const uint8_t *fb, uint8_t *out, const uint32_t *fb_clean, const DevFrame &frame, uint32_t factor,
                   hipStream_t st);
// Depth compositing: src's frame into dst's over the tiles of dst's band, by the rule of tr_composite.h and through both
// scenes' fast-clear flags: k_composite.  The caller orders the launch behind the work that produced both frames.
int launch_composite(const CompositeArgs &a, hipStream_t st);
// Shared shadows: src's shadow buffer into dst's over the tiles of the whole frame, by the rule of tr_shadow_merge.h and
// through both scenes' fast-clear flags: k_shadow_merge.  The caller orders the launch behind the work that produced
// both buffers and has made a pending clear of dst real (every flag up).
int launch_shadow_merge(const ShadowMergeArgs &a, hipStream_t st);
// Ambient occlusion: the frame's colour shaded in place from its own z buffer by the rule of tr_ao.h, through the
// scene's fast-clear flags: k_ao.  The whole frame only (no band); the caller has made the depth real.
int launch_ao(const AoArgs &a, hipStream_t st);
// Frame accumulation: a.n frames averaged under their weights into a.out over the tiles of the band, by the rule of
// tr_accumulate.h and through every frame's fast-clear flags: k_accumulate.  a.out_clean: the destination's flags when
// a.out is one of the frames (in place), else null.  The caller orders the launch behind the work that produced the frames.
int launch_accumulate(const AccumulateArgs &a, hipStream_t st);
// Depth of field: a.fb blurred by a.z into a.out (which does not overlap it) by the rule of tr_dof.h, through the scene's
// fast-clear flags of z and of colour: k_dof.  The whole frame only (no band); the caller has made the depth real.
// a.out_clean: null, or the flags of `out` the kernel writes.
int launch_dof(const DofArgs &a, hipStream_t st);
// Bloom: a.fb keyed, blurred by the tent and added back into a.out (which does not overlap it) by the rule of tr_bloom.h,
// through the scene's colour fast-clear flags: k_bloom.  The whole frame only (no band); no depth is read.
// a.out_clean: null, or the flags of `out` the kernel writes.
int launch_bloom(const BloomArgs &a, hipStream_t st);
// Colour grading: a.fb mapped through the table a.lut (n^3 packed entries, padded to whole 16-byte pieces, 16-byte
// aligned) into a.out -- a.fb itself or a buffer apart from it -- by the rule of tr_grade.h, through the frame's colour
// fast-clear flags: k_grade, persistent workgroups.  The scene's tile grid, a band's included; no depth is read.
// a.lower_clean: null, or a.fbclean (in place, c0 != 0): the flags of the tiles stored as c0 come down.
// cap: 0, or the most workgroups to start (tr_scene_debug_grade_grid); *grid: the number started (0: nothing launched).
int launch_grade(const GradeArgs &a, hipStream_t st, uint32_t cap, uint32_t *grid);
// Outlines: ink laid over a.fb where a.z has a silhouette, a depth step or a fold, into a.out -- a.fb itself or a buffer
// apart from it -- by the rule of tr_outline.h, through the scene's fast-clear flags of z and of colour: k_outline.  The
// whole frame only (no band); the caller has made the depth real.  In place the colour flag of a flagged tile the kernel
// writes comes down.
int launch_outline(const OutlineArgs &a, hipStream_t st);
// Edge anti-aliasing: a.fb filtered by the rule of tr_aa.h into a.out, which is apart from it (a pixel reads its
// neighbours), through the scene's colour fast-clear flags: k_aa.  The whole frame only (no band).  a.out_clean: null, or
// where each workgroup writes the flag of its tile of a.out -- a tile flagged there is zeros in every byte.
int launch_aa(const AaArgs &a, hipStream_t st);
// Resize: a.fb scaled to a.out (a.out_w x a.out_h, apart from it) by the rule of tr_resize.h through the tables a.x and a.y
// (device memory, built by resize_axis on the host) and the scene's colour fast-clear flags: k_resize, in the shape
// a.shape of kResizeShapes, which the vertical table must fit (a.y_span).  The whole frame only (no band); no depth is read.
int launch_resize(const ResizeArgs &a, hipStream_t st);
// Warp: a.fb resampled to a.out (a.out_w x a.out_h, apart from it) by the rule of tr_warp.h through the node grid a.grid
// (device memory; one grid, or three with a.rule.per_channel) and the scene's colour fast-clear flags: k_warp.  The whole
// frame only (no band); no depth is read.  a.out_clean: null, or -- the output has the frame's size and its height is a
// multiple of 16 -- where each workgroup writes the flag of its tile of a.out: a tile flagged there is zeros in every byte.
int launch_warp(const WarpArgs &a, hipStream_t st);
// YUV output: the rgb8 image a.src (a.width x a.height, each 1..8192) converted to the planes of a.rule.layout in a.out
// (yuv_bytes, apart from it, any address) by the rule of tr_yuv.h: k_yuv.  a.clean: null, or the image's colour
// fast-clear flags over its whole 128 x 16 tile grid (a.ntx a row).  No depth is read.
int launch_yuv(const YuvArgs &a, hipStream_t st);
// Layers: a.image (a.rule's size, format and stride; from_scene: another scene's rgb8 frame behind a.src_clean /
// a.src_all_clean) blended into a.fb at (a.rule.x, a.rule.y) by the rule of tr_layer.h, into a.out -- a.fb itself (in
// place: only the tiles the rectangle touches are launched, none where it misses) or apart from it (every tile: the
// rest is copied, a flagged tile as zeros): k_layer.  The whole frame only (no band); z and a.zclean are read only with
// a WHERE flag.  a.total, a.c* and a.g* are set here.
int launch_layer(const LayerArgs &a, bool from_scene, hipStream_t st);
// Depth ramp: a.fb blended with the entries of the table a.table (a.rule.n packed rgba entries, padded to whole 16-byte
// pieces, 16-byte aligned) chosen by a.z, into a.out -- a.fb itself or a buffer apart from it, at any byte address -- by
// the rule of tr_ramp.h, through the frame's fast-clear flags of z and of colour: k_ramp, persistent workgroups.  The
// whole frame only (no band); the caller has made the depth real.  a.lower: null, or a.fbclean (in place): the flags of
// the flagged tiles stored whole come down.  cap and *grid as for launch_grade (tr_scene_debug_ramp_grid).
int launch_ramp(const RampArgs &a, hipStream_t st, uint32_t cap, uint32_t *grid);
// Projector: the image a.image cast onto the drawn pixels of a.fb through a.rule.m, under OCCLUDE shadowed by a.occ_z
// behind a.occ_zclean, into a.out -- a.fb itself or a buffer apart from it, at any byte address -- by the rule of
// tr_projector.h, through the frame's fast-clear flags of z and of colour: k_projector, one workgroup a tile.  The whole
// frame only (no band); the caller has made both depths real.  a.lower: null, or a.fbclean (in place).
int launch_projector(const ProjectorArgs &a, hipStream_t st);
// Relight: the lights of a.rule laid on the pixels of a.fb that have a normal, recovered from a.z behind a.zclean, into
// a.out -- a.fb itself or a buffer apart from it, at any byte address -- by the rule of tr_relight.h, through the frame's
// fast-clear flags of z and of colour: k_relight, one workgroup a tile.  The whole frame only (no band); the caller has
// made the depth real.  a.lower: null, or a.fbclean (in place).
int launch_relight(const RelightArgs &a, hipStream_t st);
// Distance field: the three passes of tr_distance.h over the whole frame (no band), each its own kernel.  launch_dist_mask:
// a.mask from a.fb (KEY) or a.z (DRAWN; the caller has made the depth real) through the fast-clear flags: k_dist_mask.
// launch_dist_row: a.h and a.summary from a.mask: k_dist_row.  launch_dist: a.field (any 2-byte-aligned address) from
// a.h, a.summary and a.mask: k_dist.  launch_dist_apply: a.fb blended with the table's entries chosen by a.field (complete,
// 8-byte aligned) into a.out -- a.fb itself or apart from it --, a.lower as for launch_ramp: k_dist_apply.
int launch_dist_mask(const DistArgs &a, hipStream_t st);
int launch_dist_row(const DistArgs &a, hipStream_t st);
int launch_dist(const DistArgs &a, hipStream_t st);
int launch_dist_apply(const DistApplyArgs &a, hipStream_t st);
// Lines: the table a.lines drawn into a.fb by its per-tile lists (a.offsets, a.entries; tr_lines.h has the rule and the
// binning), into a.out -- a.fb itself or a buffer apart from it, at any byte address --, through the frame's fast-clear
// flags of colour and, under LINES_DEPTH_TEST, of z: k_lines.  The whole frame only (no band); under the test the caller
// has made the depth real.  In place one workgroup per entry of a.tiles (n_listed of them: the non-empty tiles; none, or
// opacity 0: nothing is launched); out of place one per tile.  a.lower: null, or a.fbclean (in place).
int launch_lines(const LinesArgs &a, uint32_t n_listed, hipStream_t st);
// Convolve: a.fb filtered through the integer kernel a.rule into a.out (which does not overlap it) by the rule of
// tr_convolve.h, through the scene's colour fast-clear flags: k_convolve.  The whole frame only (no band); no depth is
// read.  a.words and a.rule.mul24 are set here.  a.out_clean: null, or where each workgroup writes the flag of its tile
// of a.out -- a tile flagged there is zeros in every byte.
int launch_convolve(const ConvolveArgs &a, hipStream_t st);
// Rank: a.fb through the order-statistic filter a.rule into a.out (which does not overlap it) by the rule of tr_rank.h,
// through the scene's colour fast-clear flags: k_rank, in its extremes form where every rank asked for is the first or
// the last, else the general one.  The whole frame only (no band); no depth is read.  a.words is set here.  a.out_clean
// as for launch_convolve.
int launch_rank(const RankArgs &a, hipStream_t st);
// Bilateral: a.fb through the edge-preserving weighted mean a.rule into a.out (which does not overlap it) by the rule of
// tr_bilateral.h, through the scene's colour fast-clear flags: k_bilateral.  The whole frame only (no band).  Under the
// DEPTH guide a.z and a.zclean are read and the caller has made the depth real; under the COLOUR guide neither is.
// a.words is set here.  a.out_clean as for launch_convolve.
int launch_bilateral(const BilateralArgs &a, hipStream_t st);
// Frame statistics: the frame a.fb (and, with a.rule.depth, its depth a.z) reduced to the record of tr_stats.h through the
// frame's fast-clear flags: k_stats, persistent workgroups that each store a partial record to a slot of a.partials, then
// k_stats_finish, which sums the slots into `out` (STATS_WORDS words of device memory, or the device address of mapped
// host memory).  The scene's tile grid, a band's included; nothing of the scene is written.  a.partials holds at least
// stats_max_grid(a.frame) slots.  cap: 0, or the most workgroups to start (tr_scene_debug_stats_grid); *grid: the number
// started.
int launch_stats(const StatsArgs &a, uint32_t *out, hipStream_t st, uint32_t cap, uint32_t *grid);
// The most workgroups a k_stats launch over `frame` starts on the current device (0: the device cannot be asked).
uint32_t stats_max_grid(const DevFrame &frame);
// Dynamic textures: image a.src into the plain array a.texel and the owned words of the texel set a.set (words per texel:
// 1 or 4; a.set null: the plain array alone) by the rule of tr_pack.h, through the source's colour-clean flags when it
// is a frame: k_pack_texels.  The caller orders the launch behind whatever reads the arrays and produced the source.
int launch_pack_texels(const PackArgs &a, int words, hipStream_t st);
// Morph targets: the posed rows of n_frames frames (<= MORPH_MAX_FRAMES) by one launch -- frame f blends the mesh's
// gathered rows `base` (n_rows x TRI_FLOATS) with the gathered delta rows `delta` (n_targets x n_rows x TRI_FLOATS) under
// the weights tab.f[f].w (device memory) into tab.f[f].dst: k_morph, tr_morph.h.
int launch_morph(const float *base, const float *delta, uint32_t n_rows, uint32_t n_targets, const MorphTable &tab, uint32_t n_frames,
                 hipStream_t st, hipEvent_t start, hipEvent_t done);
// Skinning: the skinned rows of n_frames frames (<= SKIN_MAX_FRAMES) by one launch -- frame f skins the rows tab.f[f].src
// (n_rows x TRI_FLOATS; may be tab.f[f].dst) under the palette tab.f[f].pal (n_bones x 24 floats, device memory) and the
// gathered influence rows `infl` (n_rows x SKIN_ROW_WORDS) into tab.f[f].dst: k_skin, tr_skin.h.
int launch_skin(const uint32_t *infl, uint32_t n_rows, uint32_t n_bones, const SkinTable &tab, uint32_t n_frames, hipStream_t st,
                hipEvent_t start, hipEvent_t done);
int launch_selftest(const float *x, const float *d, uint32_t n, uint32_t *out_u32, int32_t *out_i32,
                    uint32_t *out_u8, float *out_div, float *out_div_ref, hipStream_t st);
// Peer exchange flags (tr_exchange.cpp): system-scope store of a generation number; waits that poll
// until flag >= value (as a wrapping distance) and raise *error after timeout_ticks of the 100 MHz wall clock
int launch_flag_store(uint32_t *flag, uint32_t value, hipStream_t st);
// ... unless *unless != 0 (the exchange's error word: a wait earlier on the queue timed out)
int launch_flag_store_unless(uint32_t *flag, uint32_t value, const uint32_t *unless, hipStream_t st);
int launch_flags_store_all(uint32_t *const *flags, uint32_t n, uint32_t skip, uint32_t value, hipStream_t st);
int launch_flag_wait(uint32_t *flag, uint32_t value, uint32_t *error, uint64_t timeout_ticks, hipStream_t st);
int launch_flags_wait_all(uint32_t *const *flags, uint32_t n, uint32_t skip, uint32_t value, uint32_t *error,
                          uint64_t timeout_ticks, hipStream_t st);
// rcp2 (which = 0) / sqrt2 (1) of tr_pk.h against '/' and sqrtf for the f32 bit patterns [first, first + count)
int launch_selftest_unary(int which, uint32_t first, uint64_t count, unsigned long long *n_bad, uint32_t *bad_bits,
                          hipStream_t st);
// shadow_fetch (tr_shaders.h) on the device: through the fast-clear flags on `stale`, and plain on `plain`
int launch_selftest_shadow(const float *plain, const float *stale, const uint32_t *sclean, uint32_t W, uint32_t H,
                           const float *x, const float *y, uint32_t n, uint32_t *out_plain, uint32_t *out_flagged,
                           uint32_t *err_plain, uint32_t *err_flagged, hipStream_t st);
// 1 when the specular closure's powf reproduces the host libm's bit for bit (tr_powf.h)
int specular_is_exact();
int launch_depth_view(const float *src, uint8_t *dst, uint32_t W, uint32_t H, hipStream_t st);

}  // namespace tr
