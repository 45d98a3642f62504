// tr_kernels.hip -- gfx950 kernels of the triangle-fill path.
//
// The reference (src/scene.rs:151-268) is one serial loop nest: pass x polygon x bbox-x x
// bbox-y, depth-testing and shading each covered pixel in polygon order.  Here a render pass is
// four kernels:
//
//   k_setup        one lane per polygon: vertex closure, clamped bounding box, the polygon's record;
//                  the wavefront then counts, per tile, the polygons whose box meets it
//   k_order        one thread per tile: the tile kernel's work lists, tiles by polygon count, and
//                  every tile's range of exactly that many records in the pass's pool
//   k_bin          copies the records into the tiles' ranges (exact binning: see k_setup below)
//   k_tile         one workgroup (4, 8 or 16 waves) per 128x16 screen tile, heaviest tiles first:
//                  the bin is copied into LDS in one coalesced pass, each wave resolves coverage +
//                  depth for its column of the tile against LDS keys, then the survivors are shaded
//                  from the LDS records and depth and colour are streamed out once, as whole cache
//                  lines; tiles without polygons only stream their cleared colour
//
// Equivalence with the serial loop: `z <= zbuf -> reject` in polygon order means the surviving
// fragment of a pixel is the one with the largest z, ties going to the lowest polygon index, and
// the frame buffer keeps the colour of the last accepted fragment = that survivor
// (shader.rs:169-180, scene.rs:259-263).  A max over (z, index) computes the same survivor in
// any order, so only survivors are shaded.  The depth-only passes use `>=` (shader.rs:703):
// largest z, ties to the highest index.
//
// No MFMA anywhere: the path is compare/gather/stream work bound by HBM writes.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdlib.h>

#include <algorithm>
#include <type_traits>

#include "tr_aa.h"
#include "tr_accumulate.h"
#include "tr_ao.h"
#include "tr_composite.h"
#include "tr_dof.h"
#include "tr_bloom.h"
#include "tr_convolve.h"
#include "tr_rank.h"
#include "tr_bilateral.h"
#include "tr_grade.h"
#include "tr_stats.h"
#include "tr_kernels.h"
#include "tr_morph.h"
#include "tr_outline.h"
#include "tr_pack.h"
#include "tr_plan.h"
#include "tr_resolve.h"
#include "tr_shaders.h"
#include "tr_skin.h"

namespace tr {

namespace {

constexpr int NBY = TILE_H / 8;  // block rows per quadrant
constexpr uint32_t NO_WINNER = 0xFFFFFFFFu;
static_assert(NBY == 2 && TILE_H % 4 == 0, "the pixel-pair code assumes two block rows per quadrant");

__device__ __forceinline__ int32_t tile_index(const DevFrame &f, int32_t tx, int32_t ty)
{
    return (ty - f.ty_base) * (int32_t)f.ntx + tx;
}

// -----------------------------------------------------------------------------------------
// k_setup
// -----------------------------------------------------------------------------------------
// Binning is EXACT: k_setup runs the vertex stage and counts, per tile, the polygons whose clamped box meets it;
// k_order gives every tile with polygons a range of exactly that many records in the pass's pool (one atomic per
// wave: tiles need no particular order in the pool); k_bin then fills the ranges.  No tile has a capacity: ten
// times the usual number of polygons in one tile is just a longer range.  What is bounded is the pool -- the
// pairs of the whole pass -- sized generously by the host and grown (the frame rendered again) should a pass ever
// exceed it.  (Round 2 gave every tile a fixed-capacity bin: 4 GiB of reservations at 4096^2 for 2.6 MB of records
// per frame, and TR_E_BIN_OVERFLOW whenever one tile saw more than its share.)
// Workgroups of the chain's kernels are FOUR independent waves: a compute unit that is full of tile-kernel
// workgroups admits a wave of another kernel only where a tile workgroup has left, and that wave -- on one SIMD --
// then keeps the next tile workgroup (a wave on every SIMD) out for as long as it lives.  Four waves that arrive
// together, one per SIMD, block that one slot once; as 64-thread workgroups the same waves blocked up to four
// slots, and the 4096^2 tile kernel ran 4 % slower beside them.  (A lone frame's chain has the machine to itself
// and is launched as single waves: they spread over four times as many compute units.)
constexpr uint32_t CHAIN_WAVES = 4;
constexpr uint32_t CHAIN_THREADS = 64 * CHAIN_WAVES;

// Polygon t's record (P pieces) for the pass `a` describes: vertex closure, truncating projection, clamped box.
// A polygon that draws nothing (culled, off screen, degenerate, t beyond the mesh) gets the canonical empty box
// (bx0 = 1 > bx1 = 0) and nothing else.  Returns the device error bits the vertex stage raised.
template <int VS, int P, bool XF>
__device__ __forceinline__ uint32_t setup_record(const SetupArgs &a, uint32_t t, uint4 (&o)[P])
{
    uint32_t err = 0;
#pragma unroll
    for (int i = 0; i < P; i++) o[i] = make_uint4(0u, 0u, 0u, 0u);
    o[0] = make_uint4(1u, 0u, 0u, 0u);
    if (t >= a.mesh.n_tri) return 0u;
    RasterRec r;
    float v[VARY_STRIDE];
#pragma unroll
    for (int i = 0; i < VARY_STRIDE; i++) v[i] = 0.0f;
    const bool keep = vertex_stage<VS, XF>(a.mesh, a.u, t, r, v, err);
    if (keep)
        finish_raster_rec(r, a.frame);
    else
        mark_rejected(r);
    // piece 0: the clamped box (coordinates below 2^15; bx0 = 1 > bx1 = 0: draws nothing) and, in a tile's copy,
    // the pair's coverage masks (pair_masks, tr_shaders.h: filled in by k_bin)
    // (a polygon that draws nothing may have any coordinates: it gets the canonical empty box)
    if (r.bx0 <= r.bx1) {
        o[0] = make_uint4((uint32_t)r.bx0 | ((uint32_t)r.bx1 << 16), (uint32_t)r.by0 | ((uint32_t)r.by1 << 16), 0u, 0u);
        // vertex 0 and the two edge vectors from it, the latter already as the f32 values every
        // pixel's to_barycentric_coord starts from (scene.rs:178-181: integer difference, then
        // the conversion) -- the tile kernel's shading phase used to redo these 8 subtractions
        // and 8 conversions for every pixel pair
        const Edge e = edge_setup(r);
        o[1] = make_uint4((uint32_t)r.x0, (uint32_t)r.y0, __float_as_uint(e.a0), __float_as_uint(e.b0));
        o[2] = make_uint4(__float_as_uint(e.a1), __float_as_uint(e.b1), __float_as_uint(r.z0), __float_as_uint(r.z1));
        o[3] = make_uint4(__float_as_uint(r.z2), t, __float_as_uint(v[0]), __float_as_uint(v[1]));
#pragma unroll
        for (int i = 4; i < P - 1; i++)
            o[i] = make_uint4(__float_as_uint(v[4 * i - 14]), __float_as_uint(v[4 * i - 13]),
                              __float_as_uint(v[4 * i - 12]), __float_as_uint(v[4 * i - 11]));
        // spare last word (varying 9 / 21 is unused): RN(1 / cross.z), the one IEEE division
        // per polygon; k_tile derives every per-pixel quotient from it (tr_math.h div_by)
        o[P - 1] = make_uint4(__float_as_uint(v[4 * (P - 1) - 14]), __float_as_uint(v[4 * (P - 1) - 13]),
                              __float_as_uint(v[4 * (P - 1) - 12]), __float_as_uint(record_recip(r)));
    }
    return err;
}

// The (polygon, tile) pairs of a wave whose lane l holds the box of one polygon (or the empty box): numbered by a
// prefix sum over the lanes, so that they can be dealt to all 64 lanes -- a polygon that spans 40 tiles is 40 lanes'
// work for one step, not one lane's loop of 40 while the others idle.
struct PairDeal {
    int32_t corner, ntx, excl, total;  // this lane's polygon: first tile column | first tile row << 16, tile columns, pairs before it
    __device__ __forceinline__ PairDeal(const uint4 &piece0)
    {
        const uint32_t lane = threadIdx.x & 63u;
        const int32_t bx0 = (int32_t)(piece0.x & 0xFFFFu), bx1 = (int32_t)(piece0.x >> 16);
        const int32_t by0 = (int32_t)(piece0.y & 0xFFFFu), by1 = (int32_t)(piece0.y >> 16);
        int32_t cnt = 0;
        corner = 0;
        ntx = 1;
        if (bx0 <= bx1) {
            corner = bx0 / TILE_W | (by0 / TILE_H) << 16;
            ntx = bx1 / TILE_W - bx0 / TILE_W + 1;
            cnt = ntx * (by1 / TILE_H - by0 / TILE_H + 1);
        }
        int32_t incl = cnt;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int32_t up = __shfl_up(incl, d, 64);
            if ((int)lane >= d) incl += up;
        }
        total = __shfl(incl, 63, 64);
        excl = incl - cnt;
    }
    // pair p (every lane of the wave calls this together; p may lie beyond `total`): the lane that holds its polygon
    // and the tile; false beyond the last pair
    __device__ __forceinline__ bool locate(int32_t p, int32_t &owner, int32_t &ptx, int32_t &pty) const
    {
        // owner = last lane whose exclusive offset is <= p (lanes without pairs share their successor's offset, so
        // "last" skips them)
        int32_t lo = 0, hi = 63;
#pragma unroll
        for (int i = 0; i < 6; i++) {
            const int32_t mid = (lo + hi + 1) >> 1;
            if (__shfl(excl, mid, 64) <= p)
                lo = mid;
            else
                hi = mid - 1;
        }
        const int32_t q = p - __shfl(excl, lo, 64), w = __shfl(ntx, lo, 64), c = __shfl(corner, lo, 64);
        owner = lo;
        ptx = (c & 0xFFFF) + q % w;
        pty = (c >> 16) + q / w;
        return p < total;
    }
};

// Bumps the counter of every tile the wave's polygons' boxes meet (atomics that return nothing: nothing waits for them).
__device__ __forceinline__ void count_tiles(const SetupArgs &a, const uint4 &piece0)
{
    const PairDeal deal(piece0);
    const int32_t lane = (int32_t)(threadIdx.x & 63u);
    for (int32_t p0 = 0; p0 < deal.total; p0 += 64) {
        int32_t owner, ptx, pty;
        if (deal.locate(p0 + lane, owner, ptx, pty))
            __hip_atomic_fetch_add(&a.tile_count[tile_index(a.frame, ptx, pty)], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// Which polygon a lane of the chain's kernels takes.  The first `polys` lanes of every wave take one each, INTERLEAVED
// over the launch's waves (lane l of wave w: polygon l * waves + w): neighbours in a mesh are neighbours on the screen
// and of similar size -- in mesh order one wave got the eight largest polygons of the reference's model and was the
// critical path of the whole chain (k_bin's waves: median 3.4 us, slowest 13).
__device__ __forceinline__ uint32_t chain_polygon(uint32_t block, uint32_t polys)
{
    const uint32_t lane = threadIdx.x & 63u, wave = block * (blockDim.x >> 6) + (threadIdx.x >> 6), waves = gridDim.x * (blockDim.x >> 6);
    return lane < polys ? lane * waves + wave : 0xFFFFFFFFu;
}

// XF: some frame of the launch draws a transform table (DevMesh::inst_xform); false: the kernel without that branch.
template <int VS, bool XF>
__device__ __forceinline__ void setup_body(const SetupArgs &a, uint32_t block, uint32_t polys)
{
    constexpr int P = (VS == VS_DARBOUX) ? REC_PIECES_LARGE : REC_PIECES_SMALL;
    // Lane = polygon: vertex closure, truncating projection, clamped box; the polygon's record goes to the pass's
    // record array ONCE (k_bin copies it to the tiles), its tiles' counters are bumped with atomics that return
    // nothing, so nothing waits for them.
    __builtin_amdgcn_s_setprio(3);  // (see k_order)
    // the 16 words behind this pass's counters (k_order's list lengths and pool cursor): their last readers --
    // the tile kernel of the pass that had the set before -- are done (the host orders that)
    if (block == 0u && threadIdx.x < 16u) a.tile_count[a.frame.ntx * a.frame.nty + threadIdx.x] = 0u;
    const uint32_t t = chain_polygon(block, polys);
    uint4 rec[P];
    const uint32_t err = setup_record<VS, P, XF>(a, t, rec);
    if (t < a.mesh.n_tri) {
        uint4 *o = reinterpret_cast<uint4 *>(a.recs) + (size_t)t * P;
        o[0] = rec[0];
        if ((rec[0].x & 0xFFFFu) <= (rec[0].x >> 16)) {
#pragma unroll
            for (int i = 1; i < P; i++) o[i] = rec[i];
        }
    }
    count_tiles(a, rec[0]);
    if (err) {
        atomicOr(a.err, err);
        *a.alarm = 1u;
    }
}

template <int VS, bool XF>
__global__ __launch_bounds__(CHAIN_THREADS) void k_setup(SetupArgs a, uint32_t polys)
{
    setup_body<VS, XF>(a, blockIdx.x, polys);
}

// k_bin: copies every polygon's record into the range of each tile its box meets, with the pair's coverage masks.
// One lane per polygon would serialise a polygon's copies (a polygon spanning 30 tiles = 30 dependent round
// trips); instead the wave's (polygon, tile) pairs are numbered by a prefix sum and dealt round-robin to the
// lanes, PAIRS per lane per trip so that their returning atomics are in flight together.  A pair's place in the
// pool comes from counting the tile's counter DOWN from the end of the tile's range (k_order left it there).
// `polys`: polygons per wave (the wave with the most pairs is the kernel's critical path, and a lone frame waits
// for it: few for a small mesh).
constexpr uint32_t BIN_POLYS = 64;

__device__ __forceinline__ uint4 shuffle_piece(const uint4 &v, int32_t from)
{
    return make_uint4((uint32_t)__shfl((int)v.x, from, 64), (uint32_t)__shfl((int)v.y, from, 64), (uint32_t)__shfl((int)v.z, from, 64),
                      (uint32_t)__shfl((int)v.w, from, 64));
}

// The wave's polygons are in its lanes' registers (`mine`: lane l holds one record, or the empty box): their
// (polygon, tile) pairs are numbered by a prefix sum and dealt to all 64 lanes, which fetch the record from the
// owner lane with shuffles (no LDS: nothing to fit beside the tile kernel's workgroups, no barrier).
template <int P>
__device__ __forceinline__ void bin_deal(const SetupArgs &a, const uint4 (&mine)[P])
{
    const int32_t lane = (int32_t)(threadIdx.x & 63u);
    const PairDeal deal(mine[0]);
    constexpr int PAIRS = 2;  // pairs per lane per trip: their atomics are in flight together
    for (int32_t p0 = 0; p0 < deal.total; p0 += 64 * PAIRS) {
        int32_t own[PAIRS], origin[PAIRS];
        uint32_t at[PAIRS];
        bool have[PAIRS];
#pragma unroll
        for (int k = 0; k < PAIRS; k++) {
            have[k] = false;
            own[k] = 0;
            if (p0 + 64 * k >= deal.total) continue;  // (uniform)
            int32_t ptx, pty;
            have[k] = deal.locate(p0 + 64 * k + lane, own[k], ptx, pty);
            if (have[k]) {
                origin[k] = ptx | pty << 16;
                at[k] = atomicSub(&a.tile_count[tile_index(a.frame, ptx, pty)], 1u) - 1u;
            }
        }
#pragma unroll
        for (int k = 0; k < PAIRS; k++) {
            if (p0 + 64 * k >= deal.total) continue;  // (uniform: every lane takes part in the shuffles)
            uint4 piece[P];
#pragma unroll
            for (int i = 0; i < P; i++) piece[i] = shuffle_piece(mine[i], own[k]);
            // (pool exhausted: k_order has raised DE_BIN_OVERFLOW, the host renders again)
            if (!have[k] || at[k] >= a.pool_cap) continue;
            uint4 *dst = reinterpret_cast<uint4 *>(a.bins) + (size_t)at[k] * P;
            // which cells (small pair) or block columns (large pair) of the box inside THIS tile can hold
            // a fragment: the tile kernel evaluates no edge function to find its work
            pair_masks((int32_t)(piece[0].x & 0xFFFFu), (int32_t)(piece[0].x >> 16), (int32_t)(piece[0].y & 0xFFFFu),
                       (int32_t)(piece[0].y >> 16), (int32_t)piece[1].x, (int32_t)piece[1].y, __uint_as_float(piece[1].z),
                       __uint_as_float(piece[2].x), __uint_as_float(piece[1].w), __uint_as_float(piece[2].y),
                       (origin[k] & 0xFFFF) * TILE_W, (origin[k] >> 16) * TILE_H, a.cells != 0u, piece[0].z, piece[0].w);
#pragma unroll
            for (int i = 0; i < P; i++) dst[i] = piece[i];
        }
    }
}

template <int P>
__device__ __forceinline__ void bin_body(const SetupArgs &a, uint32_t block, uint32_t polys)
{
    __builtin_amdgcn_s_setprio(3);  // (see k_order)
    const uint32_t t = chain_polygon(block, polys);
    // the lane's polygon, in registers
    uint4 mine[P];
#pragma unroll
    for (int i = 0; i < P; i++) mine[i] = make_uint4(0u, 0u, 0u, 0u);
    mine[0] = make_uint4(1u, 0u, 0u, 0u);
    if (t < a.mesh.n_tri) {
        const uint4 *const rec = reinterpret_cast<const uint4 *>(a.recs) + (size_t)t * P;
#pragma unroll
        for (int i = 0; i < P; i++) mine[i] = rec[i];  // (a polygon that draws nothing has only its box written: the rest is not used)
    }
    bin_deal<P>(a, mine);
}

template <int P>
__global__ __launch_bounds__(CHAIN_THREADS) void k_bin(SetupArgs a, uint32_t polys)
{
    bin_body<P>(a, blockIdx.x, polys);
}

// Read-only argument tables of the fused launches: viewed in the constant address space, so that the loads
// are scalar and invariant (a member is loaded where it is used, arrays are indexed in place) -- what the
// compiler does with kernel arguments.
template <typename T>
using constant_ptr = const __attribute__((address_space(4))) T *;

// The same for a group of frames in one launch (tr_scene_render_frames): blockIdx.y = frame, whose
// arguments are entry y of a table in device memory.
template <int VS, bool XF>
__global__ __launch_bounds__(CHAIN_THREADS) void k_setup_group(const SetupArgs *__restrict__ table, uint32_t polys)
{
    setup_body<VS, XF>(*(const SetupArgs *)((constant_ptr<SetupArgs>)table + blockIdx.y), blockIdx.x, polys);
}

template <int P>
__global__ __launch_bounds__(CHAIN_THREADS) void k_bin_group(const SetupArgs *__restrict__ table, uint32_t polys)
{
    const SetupArgs &a = *(const SetupArgs *)((constant_ptr<SetupArgs>)table + blockIdx.y);
    // the pass's list lengths (k_order has completed) to the host, which sizes later tile kernels' grids by them
    constexpr uint32_t N_LISTS = 8u;  // (ORDER_BUCKETS, below)
    if (blockIdx.x == 0u && threadIdx.x < N_LISTS && a.len_host)
        __hip_atomic_store(a.len_host + threadIdx.x, gload(a.len_src + threadIdx.x), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    bin_body<P>(a, blockIdx.x, polys);
}

// -----------------------------------------------------------------------------------------
// k_lit
// -----------------------------------------------------------------------------------------
// The normal-map and specular closures use nothing of a fragment but its texel (shade_texel, tr_shaders.h): under one
// frame's light and camera the colour of a fragment is a function of (u, v)'s texel alone.  Where a frame shades many
// more fragments than the images have texels -- the x64 grid at 8192^2: ~20 M fragments, 1 M texels -- the closure
// runs ONCE PER TEXEL here, in the chain in front of the tile kernel, and the tile kernel's fragment stage is a fetch
// from the frame's lit image (FS_LIT).  The arithmetic is the fragment stage's own -- the two-texel closure with its
// guard, the plain closure (IEEE division and square root) behind it, the exact powf: what a fragment finds is what it
// would have computed.  Thread = two texels of the scene's texel set (four-word texels in 4x2 blocks); the lit image is
// a one-word image in 8x4 blocks (tr_texels.h).
template <int FS>
__device__ __forceinline__ void lit_body(const SetupArgs &a)
{
    // two texels per thread -- neighbours in a row of a 4x2 block -- through the two-texel closure (packed arithmetic,
    // shared-reciprocal divisions: shade_texel_pair); a texel that leaves its guarded range is redone by the plain one
    const uint32_t i = (blockIdx.x * 256u + threadIdx.x) * 2u;
    const uint32_t block = i >> 3, within = i & 7u;
    const uint32_t x = (block % a.set_bpr) * 4u + (within & 3u), y = (block / a.set_bpr) * 2u + (within >> 2);
    if (x >= a.tex_w || y >= a.tex_h) return;
    const bool second = x + 1u < a.tex_w;
    const Texel4 q0 = reinterpret_cast<const Texel4 *>(a.texel_set)[i], q1 = reinterpret_cast<const Texel4 *>(a.texel_set)[i + 1u];
    const vec3 n0 = make3(bits_f32(q0.y), bits_f32(q0.z), bits_f32(q0.w)), n1 = make3(bits_f32(q1.y), bits_f32(q1.z), bits_f32(q1.w));
    PairGuard g = guard_init();
    uint32_t c0 = 0u, c1 = 0u;
    const f2 r = shade_texel_pair<FS>(a.u, q0.x & 0xFFFFFFu, q1.x & 0xFFFFFFu, make3p(mk2(n0.x, n1.x), mk2(n0.y, n1.y), mk2(n0.z, n1.z)),
                                      q0.x >> 24, q1.x >> 24, g, c0, c1);
    if (guard_bad(g, 0) || !(r.x == r.x)) c0 = shade_texel<FS>(a.u, q0.x & 0xFFFFFFu, n0, q0.x >> 24);
    if (second && (guard_bad(g, 1) || !(r.y == r.y))) c1 = shade_texel<FS>(a.u, q1.x & 0xFFFFFFu, n1, q1.x >> 24);
    const uint32_t at = packed_index(1, a.lit_bpr, x, y);  // (x even: x + 1 is the next texel of the same 8x4 block row)
    a.lit[at] = c0;
    if (second) a.lit[at + 1u] = c1;
}

template <int FS>
__global__ __launch_bounds__(256) void k_lit(SetupArgs a)
{
    lit_body<FS>(a);
}

template <int FS>
__global__ __launch_bounds__(256) void k_lit_group(const SetupArgs *__restrict__ table)
{
    lit_body<FS>(table[blockIdx.y]);
}

// -----------------------------------------------------------------------------------------
// k_order
// -----------------------------------------------------------------------------------------
// Turns the per-tile polygon counts k_setup left into the tile kernel's WORK LISTS: every tile once, as
// (tile, count), in one of eight lists by count -- >= 64, >= 32, ... , 1, and the empty tiles -- each with a
// region of its own (n_tiles entries), so that ONE sweep suffices: a wave counts its members of a list with a
// ballot, one lane per list reserves the wave's range with a single atomic, members take base + rank.  (Round 2
// needed a counting sweep first, to know where each list starts in a common array: two dependent kernels in
// front of every tile kernel.)  The tile kernel walks the lists heaviest first (longest-processing-time-first
// packing) and handles the empty tiles in batches.  Inside a list the tiles come in a hashed order: tiles that
// are neighbours on the screen cost about the same and read the same texture region -- in row-major order the
// tile kernel was 15 % slower.  A tile's counter leaves this kernel as the END of the tile's range in the pool
// (k_bin counts it down to the start; the tile's own k_tile workgroup zeroes it for the set's next pass); the 16
// words behind the counters -- the list lengths, the pool cursor -- are zeroed by k_setup's first workgroup
// earlier in the same stream.
constexpr int ORDER_BUCKETS = 8;
constexpr int ORDER_THREADS = 256;
constexpr int ORDER_EMPTY = ORDER_BUCKETS - 1;  // the list of the tiles without polygons
static_assert(ORDER_BUCKETS == 8, "k_bin_group reports eight list lengths");
// The tile kernel's WORK UNITS: one per tile with polygons (lists 0..6, heaviest first), then one per EMPTY_CHUNK
// entries of the empty list.  A workgroup per EMPTY tile -- three quarters of a 4096^2 frame of the reference's model --
// is four waves and 20 KiB of LDS dispatched to read one flag: 3.3 of a frame's 22.8 us went into dispatching them
// (measured with a grid cut behind the busy tiles, profiles/r04_notes.md).  A launch needs
// units(lengths) = busy + ceil(empty / EMPTY_CHUNK) workgroups per frame; any larger grid is correct (the surplus
// exits at once), n_tiles always suffices, and a host that knows the lengths (SetupArgs::len_host) asks for no more.
using plan::EMPTY_CHUNK;
static_assert(plan::ORDER_LISTS_ == (uint32_t)ORDER_BUCKETS, "tr_plan.h counts the lists the tile kernel walks");

// Bijection on [0, n): odd multiplications and xor-shifts are bijections on [0, 2^bits); values
// that fall outside [0, n) are walked through the same map again (cycle walking).
__device__ __forceinline__ uint32_t scatter_tile(uint32_t b, uint32_t n, uint32_t bits)
{
    const uint32_t mask = (1u << bits) - 1u, sh = (bits + 1u) >> 1;
    uint32_t x = b;
    do {
        x = (x * 0x9E3779B1u) & mask;
        x ^= x >> sh;
        x = (x * 0x85EBCA6Bu) & mask;
        x ^= x >> sh;
    } while (x >= n);
    return x;
}

__device__ __forceinline__ uint32_t order_bucket(uint32_t n)
{
    if (n == 0u) return ORDER_EMPTY;
    const uint32_t lg = 31u - (uint32_t)__builtin_clz(n);  // floor(log2 n)
    return lg >= (uint32_t)(ORDER_BUCKETS - 2) ? 0u : (uint32_t)(ORDER_BUCKETS - 2) - lg;
}

// The pool cursor: a 64-bit word among the eight words behind the list lengths (at the first 8-byte boundary) -- the
// pairs a pass WANTS may exceed 2^32 (a million polygons that each cross a large frame) even though no pool can
// hold them: ranges are formed in 64 bits and saturate, so that "how many records the pass wanted" stays meaningful
constexpr int ORDER_POOL = ORDER_BUCKETS;
__device__ __forceinline__ unsigned long long *order_pool_cursor(uint32_t *words_behind_counters)
{
    return reinterpret_cast<unsigned long long *>(((uintptr_t)(words_behind_counters + ORDER_POOL) + 7u) & ~(uintptr_t)7u);
}
__device__ __forceinline__ uint32_t saturate_u32(unsigned long long v) { return v > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)v; }

// One workgroup's share of the sweep: tiles block * ORDER_THREADS .. of the pass `a` describes; `lengths`: the eight
// list lengths (a fused launch keeps them in its table entry, a per-frame launch behind the pass's counters).
__device__ __forceinline__ void order_body(const TileArgs &a, uint32_t *lengths, uint32_t n_tiles, uint32_t bits, uint32_t block)
{
    uint32_t *const tile_count = a.tile_count;
    WorkItem *const order = const_cast<WorkItem *>(a.order);
    unsigned long long *const pool_cursor = order_pool_cursor(tile_count + n_tiles);
    const uint32_t i = block * ORDER_THREADS + threadIdx.x, lane = threadIdx.x & 63u;
    const unsigned long long below = (1ull << lane) - 1ull;
    const bool live = i < n_tiles;
    const uint32_t t = live ? scatter_tile(i, n_tiles, bits) : 0u;
    // (agent-scope load and store of the counter: inside k_chain they are what other workgroups' atomics made and will
    // count down, with no kernel boundary in between)
    const uint32_t n = live ? __hip_atomic_load(&tile_count[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
    const uint32_t bk = order_bucket(n);
    uint32_t mine = 0u, rank = 0u;
#pragma unroll
    for (int b = 0; b < ORDER_BUCKETS; b++) {
        const unsigned long long m = __ballot(live && bk == (uint32_t)b);
        if (lane == (uint32_t)b) mine = (uint32_t)__builtin_popcountll(m);
        if (bk == (uint32_t)b) rank = (uint32_t)__builtin_popcountll(m & below);
    }
    // the wave's tiles take one contiguous piece of the pool: running sum over the lanes, the waves' sums over
    // the workgroup, ONE atomic per workgroup (every tile of every frame of a group passes through this one
    // word, and a single address takes ~90 atomics per microsecond)
    unsigned long long incl = n;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long up = (unsigned long long)__shfl_up((long long)incl, d, 64);
        if ((int)lane >= d) incl += up;
    }
    const unsigned long long wave_total = (unsigned long long)__shfl((long long)incl, 63, 64);
    __shared__ unsigned long long s_total[ORDER_THREADS / 64], s_base;
    if (lane == 0u) s_total[threadIdx.x >> 6] = wave_total;
    __syncthreads();
    unsigned long long block_total = 0u, before = 0u;
#pragma unroll
    for (int w = 0; w < ORDER_THREADS / 64; w++) {
        if ((uint32_t)w < (threadIdx.x >> 6)) before += s_total[w];
        block_total += s_total[w];
    }
    // (the list atomics and the pool atomic are in flight together)
    uint32_t base = 0u;
    unsigned long long pool_base = 0u;
    if (lane < (uint32_t)ORDER_BUCKETS && mine) base = atomicAdd(&lengths[lane], mine);
    if (threadIdx.x == 0u && block_total) pool_base = atomicAdd(pool_cursor, block_total);
    if (threadIdx.x == 0u) s_base = pool_base;
    const uint32_t pos = (uint32_t)__shfl((int)base, (int)bk, 64) + rank;
    __syncthreads();
    const unsigned long long wave_base = s_base + before;
    const unsigned long long offset = wave_base + (incl - n);
    if (lane == 0u && wave_total && wave_base + wave_total > a.pool_cap) {
        // the pass wants more records than the pool holds: the frame is truncated, the host grows the pools to at
        // least what has been asked for so far and renders again
        atomicOr(a.err, (uint32_t)DE_BIN_OVERFLOW);
        *a.alarm = 1u;
        atomicMax(a.bin_need, saturate_u32(wave_base + wave_total));
        atomicMin(a.overflow_seq, a.pass_seq);
    }
    if (live) {
        WorkItem w;
        w.tile = t;
        // a tile whose range leaves the pool: what fits (k_bin writes no further)
        w.count = offset >= a.pool_cap ? 0u : min(n, a.pool_cap - (uint32_t)offset);
        w.offset = saturate_u32(offset);
        w.pad = 0u;
        order[(size_t)bk * n_tiles + pos] = w;
        // k_bin counts the tile's counter down from the END of its range: what an atomic returns is the record's
        // place in the pool (a place beyond the pool -- pools hold fewer than 2^31 records -- is not written); the
        // tile kernel's workgroup for the tile zeroes the counter for the set's next pass
        if (n) __hip_atomic_store(&tile_count[t], saturate_u32(offset + n), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// `group` != null: blockIdx.y = frame of a group, whose counters, work lists and pool are in entry y of the tile
// kernel's argument table; else `one` describes the pass.
__global__ __launch_bounds__(ORDER_THREADS) void k_order(TileArgs one, uint32_t n_tiles, uint32_t bits, const TileArgs *__restrict__ group)
{
    // The chain in front of a tile kernel is a few hundred waves that share their SIMDs with six tile-kernel waves
    // each -- at equal priority every instruction of theirs waits its turn behind six others, and the NEXT pass's
    // tile kernel waits for them.  They are raised: the tile kernel hardly notices a few hundred short waves.
    __builtin_amdgcn_s_setprio(3);
    const TileArgs &a = group ? group[blockIdx.y] : one;
    // (a fused launch's list lengths live in its table entry, zeroed by the host with the table)
    uint32_t *const lengths = group ? const_cast<uint32_t *>(group[blockIdx.y].list_len) : a.tile_count + n_tiles;
    order_body(a, lengths, n_tiles, bits, blockIdx.x);
}

// -----------------------------------------------------------------------------------------
// k_tile
// -----------------------------------------------------------------------------------------

// LDS index of pixel (qx, qy) of a quadrant: block-major, so that during coverage lane l of a
// wave touches slot (block*64 + l): conflict-free 8-byte accesses.
// Inside a block the rows are exchanged by the block's column within its 32-pixel strip (row ^ column & 3): the shading
// phase reads a ROW of 32 keys per half-wave -- four blocks' eight-key pieces, which without the exchange start in the
// same bank (blocks are 512 bytes apart): a four-way conflict on every survivor read, 1.7 M of the headline launch's
// 2.8 M conflict cycles.  During coverage a wave's 64 lanes still cover exactly one block: any order of its rows is
// conflict-free there.
#ifndef TR_KEY_SWIZZLE
#define TR_KEY_SWIZZLE 1
#endif
__device__ __forceinline__ uint32_t key_row_swizzle(uint32_t tx)  // tx: x within the tile
{
    return TR_KEY_SWIZZLE ? ((tx >> 3) & 3u) << 3 : 0u;
}
template <int QUAD>
__device__ __forceinline__ uint32_t key_slot(uint32_t tx, uint32_t qy)
{
    constexpr int NBX = QUAD / 8, QPIX = QUAD * TILE_H;
    const uint32_t qx = tx % (uint32_t)QUAD;
    return (tx / (uint32_t)QUAD) * (uint32_t)QPIX + (((qy >> 3) * NBX + (qx >> 3)) << 6) + ((((qy & 7u) << 3) + (qx & 7u)) ^ key_row_swizzle(tx));
}

// Key layout of the SHARED resolve: row-major, the 8-pixel groups of a row rotated by the row number.
// Pixels x and x + 1 (x even) are neighbours -- a scan-line item reads both keys with one 16-byte
// access -- and a wave that sweeps a block column (lane = 8 x 8 pixels) still touches every bank once.
__device__ __forceinline__ uint32_t shared_key_slot(uint32_t tx, uint32_t qy)
{
    return qy * (uint32_t)TILE_W + (tx ^ ((qy & 7u) << 3));
}

// Streams the cleared value of a tile (scene.rs:128-137 folded into the render): z / shadow =
// f32::MIN, rgb = 0.  Whole-tile rows are whole cache lines; 16 B per lane when width % 16 == 0.
template <bool DEPTH, int TILE_THREADS, bool WINNER>
__device__ __forceinline__ void write_cleared_tile(const TileArgs &a, int32_t tile_x0, int32_t tile_y0,
                                                   bool with_depth)
{
    const int32_t W = (int32_t)a.frame.width, H = (int32_t)a.frame.height;
    const uint32_t tid = threadIdx.x;
    float *depth = DEPTH ? a.shadow : a.zbuf;
    if (a.aligned16) {
        const uint4 zmin = make_uint4(TR_F32_MIN_BITS, TR_F32_MIN_BITS, TR_F32_MIN_BITS, TR_F32_MIN_BITS);
        // depth: TILE_H rows x 32 pieces of 16 B
        for (uint32_t c = tid; c < (uint32_t)TILE_H * 32u && with_depth; c += (uint32_t)TILE_THREADS) {
            const int32_t y = tile_y0 + (int32_t)(c >> 5), x = tile_x0 + (int32_t)(c & 31u) * 4;
            if (x < W && y >= a.frame.band_y0 && y < a.frame.band_y1)
                *reinterpret_cast<uint4 *>(depth + (size_t)y * W + x) = zmin;
        }
        if (!DEPTH) {
            const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
            // colour: TILE_H rows x 24 pieces of 16 B
            for (uint32_t c = tid; c < (uint32_t)TILE_H * 24u; c += (uint32_t)TILE_THREADS) {
                const int32_t y = tile_y0 + (int32_t)(c / 24u);
                const int32_t xb = tile_x0 * 3 + (int32_t)(c % 24u) * 16;
                if (xb < W * 3 && y >= a.frame.band_y0 && y < a.frame.band_y1)
                    *reinterpret_cast<uint4 *>(a.fb + (size_t)(H - 1 - y) * W * 3 + xb) = zero;
            }
            if (WINNER && a.winner) {
                const uint4 none = make_uint4(NO_WINNER, NO_WINNER, NO_WINNER, NO_WINNER);
                for (uint32_t c = tid; c < (uint32_t)TILE_H * 32u; c += (uint32_t)TILE_THREADS) {
                    const int32_t y = tile_y0 + (int32_t)(c >> 5), x = tile_x0 + (int32_t)(c & 31u) * 4;
                    if (x < W && y >= a.frame.band_y0 && y < a.frame.band_y1)
                        *reinterpret_cast<uint4 *>(a.winner + (size_t)y * W + x) = none;
                }
            }
        }
    } else {
        for (uint32_t p = tid; p < (uint32_t)(TILE_W * TILE_H); p += (uint32_t)TILE_THREADS) {
            const int32_t y = tile_y0 + (int32_t)(p / TILE_W), x = tile_x0 + (int32_t)(p % TILE_W);
            if (x < W && y >= a.frame.band_y0 && y < a.frame.band_y1) {
                if (with_depth) depth[(size_t)y * W + x] = bits_f32(TR_F32_MIN_BITS);
                if (!DEPTH) {
                    uint8_t *px = a.fb + ((size_t)(H - 1 - y) * W + x) * 3;
                    px[0] = 0;
                    px[1] = 0;
                    px[2] = 0;
                    if (WINNER && a.winner) a.winner[(size_t)y * W + x] = NO_WINNER;
                }
            }
        }
    }
}

// Keeps a wave-uniform value in scalar registers from this point on.  A member of the argument table is an invariant
// scalar load the compiler prefers to REPEAT next to each use -- inside the shading loop that was 14 loads per step,
// each with its own s_waitcnt (band rows four times, the texture's size, pitch and address twice): a round trip to
// the scalar cache in the wave's serial path every few dozen instructions.  An empty asm makes the value opaque.
#define TR_KEEP_SCALAR(x) asm volatile("" : "+s"(x))

__device__ __forceinline__ int32_t bcast(uint32_t v, uint32_t lane)
{
    return __builtin_amdgcn_readlane((int)v, (int)lane);
}

// Waves per SIMD each k_tile variant is compiled for (= its VGPR budget: 8 -> 64, 6 -> 80, 5 -> 96,
// 4 -> 128).  Six for the light closures (walked both ways in round 1: five lost 5 %, seven lost 9 %);
// the closures that run two pixels' normalisations and a 3x3 inverse in packed registers need more
// room than that leaves them (80 VGPRs: 30-50 spilled dwords per lane, specular 446 -> 559 us on the
// x64 grid): normal_map and specular five waves (96), darboux four (128) -- profiles/r02_notes.md.
#ifndef TR_WPE_SPECULAR
#define TR_WPE_SPECULAR 5
#endif
#ifndef TR_WPE_DARBOUX
#define TR_WPE_DARBOUX 4
#endif
#ifndef TR_WPE_NORMAL_MAP
#define TR_WPE_NORMAL_MAP 6
#endif
#ifndef TR_WPE_LIGHT
#define TR_WPE_LIGHT 6
#endif
// The fused launches' kernels (GROUP) load their arguments from the table where they are used and spill far fewer
// scalar registers into vector ones (specular: 16-22 against 101-120), which is what the closures' budgets had been
// paying for: there specular fits six waves (x64 grid 349.9 -> 335.8 us per frame, 4096^2 45.0 -> 42.6) and darboux
// five (52.3 -> 48.6).
#ifndef TR_WPE_SPECULAR_GROUP
#define TR_WPE_SPECULAR_GROUP 6
#endif
#ifndef TR_WPE_DARBOUX_GROUP
#define TR_WPE_DARBOUX_GROUP 5
#endif
// Round 4: with the depth stores and the accumulate paths compiled out, the fused kernels of the light closures need
// 62 vector registers -- and a wave of the tile kernel spends nine tenths of its life waiting (LDS, the staged bin, its
// texels, two barriers): MORE waves per SIMD pay where round 1's register-starved kernels lost (seven: - 9 %).  What
// limits a four-wave tile's workgroups per compute unit beyond six is LDS: 16 KiB of keys + 8 KiB of resident records;
// with fewer resident records (lds_rec_bytes below: 72 at seven workgroups per CU, 40 at eight -- a tile of the reference's
// model holds six on average at 4096^2; larger bins take the chunked path as before) seven or eight fit.  Same box, 4096^2,
// k_tile per frame at 6 / 7 / 8: phong 25.3 / 23.9 / 23.6; shadow's colour pass 34.2 / 32.1 / 36.1 (64 registers: spills);
// its depth pass 29.7 / 28.1 / 27.1.  Only four-wave tiles of fused launches: tiles with eight waves are at their LDS
// limit already and lose registers (2048^2: 8.65 -> 9.05).
#ifndef TR_WPE_LIGHT_GROUP
#define TR_WPE_LIGHT_GROUP 8
#endif
#ifndef TR_WPE_SHADOW_GROUP
#define TR_WPE_SHADOW_GROUP 7
#endif
#ifndef TR_WPE_DEPTH_GROUP
#define TR_WPE_DEPTH_GROUP 8
#endif
#ifndef TR_WPE_LIT_GROUP
#define TR_WPE_LIT_GROUP 8
#endif
// (the fetch-only fragment stage of the lit texel path: specular 4096^2, columns, 6 / 7 / 8: 30.1 / 29.2 / 28.7 us per step;
// the x64 grid at 8192^2, SHARED resolve -- whose scan-line sums take another KiB of LDS, 31 resident records at eight --
// 203.4 / 198.4 / 203.0: the shared resolve stops at seven)
#ifndef TR_WPE_SHARED_MAX
#define TR_WPE_SHARED_MAX 7
#endif
// (occlusion's colour pass -- seventeen shadow-buffer lookups per fragment, 60 registers in the fused kernel: 6 / 7 / 8:
// 191 / 180 / 171 us per frame at 4096^2; the per-frame kernels of the light closures, which hold their arguments in
// registers: seven -- the unfused loop 34.2 -> 33.0)
#ifndef TR_WPE_OCCL_GROUP
#define TR_WPE_OCCL_GROUP 8
#endif
#ifndef TR_WPE_LIGHT4
#define TR_WPE_LIGHT4 7
#endif
// Closures whose tile kernels run their per-pixel arithmetic on plain scalar pairs instead of packed ones (tr_pk.h, f2s):
// a bit per FsKind (coverage, barycentrics, uv; a two-pixel closure itself is written for the packed type and stays packed).
#ifndef TR_SCALAR_FS
#define TR_SCALAR_FS ((1 << FS_DEFAULT) | (1 << FS_PHONG) | (1 << FS_LIT) | (1 << FS_SHADOW2) | (1 << FS_NORMAL_MAP) | (1 << FS_SPECULAR))
#endif
constexpr bool tile_scalar_pairs(int fs) { return ((TR_SCALAR_FS) >> fs & 1) != 0; }
constexpr int tile_waves_per_eu(int fs, int tile_waves, bool group = false, bool shared = false)
{
    int want = fs == FS_DARBOUX ? (group ? TR_WPE_DARBOUX_GROUP : TR_WPE_DARBOUX)
               : fs == FS_SPECULAR ? (group ? TR_WPE_SPECULAR_GROUP : TR_WPE_SPECULAR)
               : fs == FS_NORMAL_MAP ? TR_WPE_NORMAL_MAP : TR_WPE_LIGHT;
    if (!group && tile_waves == 4 && fs != FS_DARBOUX && fs != FS_SPECULAR && fs != FS_NORMAL_MAP) want = TR_WPE_LIGHT4;
    if (group && tile_waves == 4) {
        if (fs == FS_DEFAULT || fs == FS_PHONG) want = TR_WPE_LIGHT_GROUP;
        if (fs == FS_SHADOW2) want = TR_WPE_SHADOW_GROUP;
        if (fs == FS_DEPTH) want = TR_WPE_DEPTH_GROUP;
        if (fs == FS_LIT) want = TR_WPE_LIT_GROUP;
        if (fs == FS_OCCLUSION2) want = TR_WPE_OCCL_GROUP;
        if (shared && want > TR_WPE_SHARED_MAX) want = TR_WPE_SHARED_MAX;
    }
    // sixteen waves per tile: a workgroup brings four waves to every SIMD, so 8 (two workgroups per
    // CU) or 4 (one) are the only useful budgets
    if (tile_waves == 16) return want >= 6 ? 8 : 4;
    return want;
}
// Bytes of a tile's bin that stay resident in LDS: what the workgroups of a compute unit leave of its 160 KiB beside
// their keys (16 KiB) and, in the shared resolve, the scan-line sums (4 B per thread + per wave).  Four-wave tiles:
// as many workgroups per CU as waves per SIMD.
constexpr int lds_rec_bytes_for(int tile_waves, int waves_per_eu, bool shared)
{
    if (tile_waves != 4) return lds_rec_bytes(tile_waves);
    // (a workgroup's share, rounded down to a multiple of 2 560 B: whatever the allocation granule -- 512 B, 1 280 B --
    // the workgroups' rounded-up allocations then still fit)
    const int per_wg = 160 * 1024 / waves_per_eu / 2560 * 2560;
    const int left = per_wg - TILE_W * TILE_H * 8 - (shared ? 4 * 64 * tile_waves + 4 * tile_waves : 8) - 64;
    const int cap = lds_rec_bytes(4);
    return (left < cap ? left : cap) / 16 * 16;
}

// Keys of the SHARED resolve (below): one 64-bit word per pixel, compared as an unsigned integer by
// an LDS atomic maximum.  High half: the depth as an order-preserving integer (-0.0 folded onto +0.0:
// the reference's `z <= zbuf` treats them as equal).  Low half: who wins among equal depths --
//   a colour fragment: (2^20 - 1 - polygon id) << 12 | bin slot + 1   -> the lowest polygon index
//   what the buffer held before the pass: all ones in a colour pass (`z <= zbuf` rejects: it beats
//   every fragment of equal depth), zero in a depth pass (`z >= shadow` accepts: it loses)
// Field limits: polygon ids below 2^20, bin slots below 4093 (launch_tile falls back to the column
// mode beyond them).
constexpr uint32_t SHARED_MAX_POLYGONS = 1u << 20, SHARED_MAX_SLOTS = 4093u;
// Shared resolve: small polygons (pair_masks, tr_shaders.h) are resolved as scan-line items (k_tile);
// 0 = every polygon is visited by a whole wave (round 2's only form).
#ifndef TR_SCAN_ITEMS
#define TR_SCAN_ITEMS 1
#endif
// (round 4: the survivor's key read whole, profiles/r04_notes.md)
#ifndef TR_KEY_B64
#define TR_KEY_B64 1
#endif
// (a depth pass stores the depth its resolve compared: k_tile, shade_steps)
#ifndef TR_DEPTH_FROM_KEYS
#define TR_DEPTH_FROM_KEYS 1
#endif
constexpr bool SCAN_ITEMS = TR_SCAN_ITEMS != 0;
// Measurement builds only (wrong frames): leave a phase out to time the others (profiles/r03_notes.md)
#ifndef TR_DBG_SKIP
#define TR_DBG_SKIP 0  // 1: no fragment stage, 2: no item passes, 4: no visits
#endif
__device__ __forceinline__ uint32_t depth_order_bits(float z)
{
    uint32_t b = __float_as_uint(z);
    b = b == 0x80000000u ? 0u : b;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// SHARED = false: every wave owns a column of the tile (32 / 16 / 8 pixels wide) and sees the whole
// bin; its pixels' keys are private, plain LDS reads and writes.
// SHARED = true: every wave sees the whole tile and owns an interleaved share of the BIN (record j
// belongs to wave j mod waves); keys are shared and updated with 64-bit LDS atomic maxima.  Waves then
// carry equal loads wherever the polygons cluster (the eyes of a head at 800^2: one 8-pixel column
// held 80 of a tile's 120 polygons and its wave ran 20 us while the others idled), and a polygon is
// visited once per tile instead of once per column it touches.
#define TR_TILE_KERNEL_ATTRS \
    __global__ __launch_bounds__(64 * TILE_WAVES) \
        __attribute__((amdgpu_waves_per_eu(tile_waves_per_eu(FS, TILE_WAVES, MODE != 0, SHARED), tile_waves_per_eu(FS, TILE_WAVES, MODE != 0, SHARED))))

// GROUP = false: one frame, arguments by value.
// GROUP = true: a fused launch over a group of n_frames frames (tr_scene_render_frames): workgroup b renders
// entry b / n_frames of the work list of frame b % n_frames, whose arguments are entry b % n_frames of a
// table in device memory -- so the heavy tiles of ALL the frames come first and the light and empty ones
// fill the slots they free: one frame's drain (a third of a lone 4096^2 launch runs on a machine that is
// emptying, and a small frame never fills it at all) is the next frame's start.
// MODE 0: one frame, arguments by value; what the pass writes is TileArgs::store, looked up at run time (the depth-only
// repeat of a colour pass is such a launch).  MODE 1 / 2: a fused launch; 2 = transient depth, decided at COMPILE time --
// a run-time flag skipped the stores but kept the arithmetic behind them (the survivors' z, the depth addresses), and
// with it the gain (same box: 28.5 -> 28.3 us per frame against 27.4 for the compiled-out form).
// INTERIOR: every frame of the launch is made of whole tiles only (tile_frame_is_interior below: the width a multiple
// of TILE_W, the band whole tile rows inside the frame), decided by the launcher for the whole launch.  Every pixel of
// every tile is then inside frame and band, so the per-pixel "is this pixel mine" tests of the shading steps (col_live,
// row_live, live, cdw_live), the byte-store arm of frames whose width is no multiple of 4 and the scalar registers
// pinned for the band's rows are not compiled at all.  Only the four-wave column kernels of fused launches have the form.
template <int FS, int TILE_WAVES, bool SHARED, int MODE, bool INTERIOR = false>
TR_TILE_KERNEL_ATTRS void k_tile(TileArgs args, const TileArgs *__restrict__ table, uint32_t n_frames)
{
    constexpr bool GROUP = MODE != 0;
    static_assert(!INTERIOR || (GROUP && !SHARED && TILE_WAVES == 4), "the interior form exists for the fused four-wave column kernels");
    static_assert(TILE_WAVES == 4 || TILE_WAVES == 8 || TILE_WAVES == 16, "a wave covers a 32, 16 or 8 pixel wide column of the tile");
    constexpr int TILE_THREADS = 64 * TILE_WAVES;
    constexpr int QUAD_COLUMN = TILE_W / TILE_WAVES;  // width of a wave's column when columns are owned
    constexpr int WAVES_PER_STRIP = TILE_WAVES / (TILE_W / STRIP);  // shading: waves sharing a 32-pixel strip
    constexpr int STRIP_ROWS = TILE_H / WAVES_PER_STRIP;            // rows of the strip each of them shades
    static_assert(STRIP_ROWS % 4 == 0, "a shading step covers four rows");
    constexpr bool DEPTH = (FS == FS_DEPTH);
    constexpr int P = (FS == FS_DARBOUX) ? REC_PIECES_LARGE : REC_PIECES_SMALL;
    constexpr int NMAX = lds_rec_bytes_for(TILE_WAVES, tile_waves_per_eu(FS, TILE_WAVES, MODE != 0, SHARED), SHARED) / (P * 16);  // records resident in LDS
    // the per-pixel arithmetic on plain pairs of scalars, or packed (tr_pk.h): per closure, measured
    using V2 = std::conditional_t<tile_scalar_pairs(FS), f2s, f2>;

    // Per pixel, column mode: .x = z of the best fragment so far (f32 bits; compared as floats, so
    // -0.0 and +0.0 tie exactly like the reference's `z <= zbuf`), .y = its bin slot + 1 (0 = "what
    // the buffer held before this pass").  Shared mode: the 64-bit key described above (.y = depth
    // order bits, .x = tie-break word whose low 12 bits are the bin slot + 1).
    __shared__ uint2 s_key[TILE_W * TILE_H];
    __shared__ uint4 s_rec[NMAX * P];
    // shared resolve: running sums of the scan-line items per thread, and per wave
    __shared__ uint32_t s_incl[SHARED ? TILE_THREADS : 1];
    __shared__ uint32_t s_wtot[SHARED ? TILE_WAVES : 1];

    // One workgroup per tile and frame, in the order of the work lists (k_order): blockIdx = b * n_frames + f is
    // entry b of frame f's lists walked heaviest first, so that the heavy tiles of ALL frames of a group are
    // dispatched first -- the long, VALU-bound ones (longest-processing-time-first packing by the hardware's
    // own dispatcher, and the machine is full of them from the first microsecond) -- then the light ones and
    // the empty tiles, whose workgroups only check flags or stream the cleared colour of a fresh frame: short
    // work that fills the slots the busy tiles free.  Measured alternatives: interleaving the two kinds, or
    // letting the busy blocks issue those stores themselves, was 5-10 % slower (profiles/r01_notes.md); fewer
    // workgroups that each take several tiles (a loop around this body) cost registers -- 7-13 spilled
    // vector registers in the light closures' kernels -- and 4-12 % (profiles/r03_notes.md).  Any order is correct.
    const uint32_t n_fr = GROUP ? n_frames : 1u;
    const uint32_t frame_of_group = blockIdx.x % n_fr;
    // (the table entry is not copied: a member is loaded where it is used, arrays are indexed in place)
    // (a fused-mode launch of ONE frame -- a per-frame pass that starts from cleared targets, launch_tile's `fused_single` --
    // has no table in memory: its arguments are `args`, the kernel's first parameter, read in place in the kernel-argument
    // segment like a table entry)
    const TileArgs &a = GROUP ? *(const TileArgs *)(table ? (constant_ptr<TileArgs>)table + frame_of_group
                                                         : (constant_ptr<TileArgs>)__builtin_amdgcn_kernarg_segment_ptr())
                              : args;
    // a fused launch has the eight lengths in its table entry, a per-frame launch (fused-mode or not) behind the pass's
    // counters (one more scalar load)
    const bool table_lengths = GROUP && table != nullptr;
    // (every frame of a fused launch starts from cleared targets and has no winner tap -- run_group, tr_scene.cpp: known
    // when the kernel is compiled, so the accumulate paths and the tap's stores are not even there)
    const bool fresh = GROUP || a.fresh != 0u;
    const bool st_z = FS == FS_DEPTH || (MODE == 0 ? (a.store & TR_STORE_DEPTH) != 0u : MODE == 1);
    const bool st_c = FS == FS_DEPTH || MODE != 0 || (a.store & TR_STORE_COLOR) != 0u;
    const uint32_t n_tiles = a.frame.ntx * a.frame.nty;
    // Work units (EMPTY_CHUNK above): workgroup blockIdx / frames of a frame takes that unit.  (A loop that lets a
    // workgroup take further units -- so that ANY grid would do and the host could size it by an estimate -- costs the
    // body registers it does not have: 48-68 bytes of spills per lane in the light closures' kernels, 22.7 -> 29.1 us per
    // frame with one workgroup per tile and 23.6 with the estimate; profiles/r04_notes.md.  So the grid is exact or full.)
    const uint32_t tid = threadIdx.x;
    __shared__ uint32_t s_stale[EMPTY_CHUNK];  // empty chunk: tile + 1 of the chunk's tiles whose colour must be written, else 0
    uint32_t entry = blockIdx.x / n_fr;
    uint32_t list = 0u;
    {
        // which list, which entry: a fused launch has the eight lengths in its table entry, a per-frame launch
        // behind the pass's counters (one more scalar load)
        constant_ptr<uint32_t> lengths = table_lengths ? (constant_ptr<uint32_t>)a.list_len : (constant_ptr<uint32_t>)a.tile_count + n_tiles;
#pragma unroll
        for (int b = 0; b < ORDER_BUCKETS - 1; b++) {
            const uint32_t len = lengths[b];
            if (list == (uint32_t)b && entry >= len) {
                entry -= len;
                list = (uint32_t)b + 1u;
            }
        }
    }
    uint64_t *const stamps = frame_of_group == 0u ? a.stamps : nullptr;  // the diagnostic stamps follow a group's first frame
    if (list == (uint32_t)ORDER_EMPTY) {
        // ---- a chunk of the empty list: EMPTY_CHUNK tiles without polygons (work unit `entry` behind the busy tiles) ----
        constant_ptr<uint32_t> lens = table_lengths ? (constant_ptr<uint32_t>)a.list_len : (constant_ptr<uint32_t>)a.tile_count + n_tiles;
        const uint32_t n_empty = lens[ORDER_EMPTY], first = entry * EMPTY_CHUNK;
        if (first >= n_empty || !fresh) return;  // (surplus workgroup of a grid sized for the worst case; an accumulating render leaves empty tiles alone)
        const uint32_t cnt = min(EMPTY_CHUNK, n_empty - first);
        // An empty tile of a cleared frame: its colour is zeros -- stored unless the tile's memory already holds them
        // (it was empty the last time it was written, too: most of a frame, most of the time); its z stays unwritten
        // behind the tile's fast-clear flag (depth passes write their f32::MIN).  (A pass that leaves the colour or the
        // depth out -- TileArgs::store -- leaves the respective memory and flags of the tile alone.)
        uint32_t my_tile = 0u;
        bool my_stale = false;
        if (tid < cnt) {
            my_tile = a.order[(size_t)ORDER_EMPTY * n_tiles + first + tid].tile;
            my_stale = st_c && (DEPTH ? a.zclean == nullptr : (a.fbclean == nullptr || gload(a.fbclean + my_tile) == 0u));
            s_stale[tid] = my_stale ? my_tile + 1u : 0u;
        }
        // (every flag has been read before the first one is raised)
        __syncthreads();
        for (uint32_t i = 0; i < cnt; i++) {
            const uint32_t t1 = s_stale[i];
            if (t1 == 0u) continue;
            const uint32_t t = t1 - 1u;
            write_cleared_tile<DEPTH, TILE_THREADS, !GROUP>(a, (int32_t)(t % a.frame.ntx) * TILE_W,
                                      (a.frame.ty_base + (int32_t)(t / a.frame.ntx)) * TILE_H, a.zclean == nullptr);
        }
        if (tid < cnt) {
            if (!DEPTH && my_stale && a.fbclean) a.fbclean[my_tile] = 1u;
            if (a.zclean && st_z) a.zclean[my_tile] = 1u;
        }
        return;
    }
    const WorkItem work = a.order[(size_t)list * n_tiles + entry];
    const uint32_t tile = work.tile;
    uint32_t n = work.count;
    // (k_bin has counted the tile's counter down to the start of its range; the set's next pass counts from zero)
    if (tid == 0u) a.tile_count[tile] = 0u;
    if (n == 0u) {
        if (fresh) {
            // an empty tile of a cleared frame: its colour is zeros -- stored unless the tile's memory
            // already holds them (it was empty the last time it was written, too: most of a frame,
            // most of the time); its z stays unwritten behind the tile's fast-clear flag (depth passes
            // write their f32::MIN).  (A pass that leaves the colour or the depth out -- TileArgs::store -- leaves the
            // respective memory and flags of the tile alone.)
            const bool stale = st_c && (DEPTH || a.fbclean == nullptr || a.fbclean[tile] == 0u);
            // every wave has read the flag before the first one raises it (a wave that came late would find
            // it up and leave its share of the tile unwritten)
            __syncthreads();
            if (stale) {
                write_cleared_tile<DEPTH, TILE_THREADS, !GROUP>(a, (int32_t)(tile % a.frame.ntx) * TILE_W,
                                          (a.frame.ty_base + (int32_t)(tile / a.frame.ntx)) * TILE_H, a.zclean == nullptr);
                if (!DEPTH && tid == 0u && a.fbclean) a.fbclean[tile] = 1u;
            }
            if (tid == 0u && a.zclean && st_z) a.zclean[tile] = 1u;
        }
        return;
    }
    const int32_t tx = (int32_t)(tile % a.frame.ntx);
    const int32_t ty = a.frame.ty_base + (int32_t)(tile / a.frame.ntx);
    const int32_t tile_x0 = tx * TILE_W, tile_y0 = ty * TILE_H;
    int32_t W = (int32_t)a.frame.width, H = (int32_t)a.frame.height;
    // what every shading step reads of the frame's arguments: into scalar registers once (TR_KEEP_SCALAR)
    // (an interior frame: the band's rows and aligned4 are never read -- no load, no register)
    int32_t band_y0 = 0, band_y1 = 0;
    uint32_t aligned4 = 1u;
    uint8_t *fb = a.fb;
    DevTextures tex = a.tex;
    TR_KEEP_SCALAR(W); TR_KEEP_SCALAR(H);
    if constexpr (!INTERIOR) {
        band_y0 = a.frame.band_y0;
        band_y1 = a.frame.band_y1;
        aligned4 = a.aligned4;
        TR_KEEP_SCALAR(band_y0); TR_KEEP_SCALAR(band_y1); TR_KEEP_SCALAR(aligned4);
    }
    TR_KEEP_SCALAR(fb);
    TR_KEEP_SCALAR(tex.packed); TR_KEEP_SCALAR(tex.packed_bpr); TR_KEEP_SCALAR(tex.w[0]); TR_KEEP_SCALAR(tex.h[0]);
    // the wave index is uniform: say so, so that quadrant bounds and the block loop stay scalar
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6)), lane = tid & 63u;

    // Diagnostic builds of a scene (TR_OPT_TILE_STAMPS) record when each busy tile ran; the stamps
    // go to a buffer of their own and nothing is computed from them.
    uint64_t t_start = 0, t_staged = 0;
    if (stamps) t_start = wall_clock64();

    float *depth = DEPTH ? a.shadow : a.zbuf;
    // is every z of this tile logically f32::MIN (cleared frame, or fast-clear flag still set)?
    // then nothing is read and every live z is written, after which the flag is down
    const bool zfresh = fresh || (a.zclean && a.zclean[tile] != 0u);
    const int32_t qy0 = tile_y0;
    constexpr uint32_t PREV_TAG = DEPTH ? 0u : 0xFFFFFFFFu;  // shared mode: tie-break word of the buffer's old content
    // A launch compiled for the shared resolve still gives tiles with few polygons to the column form:
    // sharing deals whole polygons to waves, and four polygons that each cross the entire tile would
    // occupy four waves for 16 column pairs each while the others idle (2048^2: such tiles were the
    // slowest of the frame, 19-21 us); columns split exactly that work evenly.
    const bool shared_tile = SHARED && n >= 2u * (uint32_t)TILE_WAVES && n <= SHARED_MAX_SLOTS;  // (the key's slot field)
    const int32_t lx = (int32_t)(lane & 7u), ly = (int32_t)(lane >> 3);
    const uint4 *bin = reinterpret_cast<const uint4 *>(a.bins) + (size_t)work.offset * P;  // the tile's records in the pool
    const bool resident = n <= (uint32_t)NMAX;  // the whole bin stays in LDS through shading
    // the same address for the scalar loads of the coverage visits (uniform, but loaded into vector registers)
    const uint64_t bin_addr = reinterpret_cast<uint64_t>(bin);
    const constant_ptr<uint32_t> bin_s = (constant_ptr<uint32_t>)(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(bin_addr >> 32)) << 32) |
                                                            (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)bin_addr));

    // ---- initial keys, coverage + depth resolve: one body for both forms ------------------------
    auto resolve = [&](auto shared_tag) {
        constexpr bool SH = decltype(shared_tag)::value;
        constexpr int QUAD = SH ? TILE_W : QUAD_COLUMN;  // width of the region a wave resolves
        constexpr int NBX = QUAD / 8;                    // 8x8 lane blocks per row of it
        constexpr int QPIX = QUAD * TILE_H;
        const int32_t qx0 = SH ? tile_x0 : tile_x0 + (int32_t)wave * QUAD;
        uint2 *wkey = SH ? s_key : s_key + wave * QPIX;
        // What the resolve reads of W, H and the band: only the guards of the initial keys' depth loads below, which
        // exist for an accumulating render (!zfresh) -- a fused launch, and with it every INTERIOR kernel, starts from
        // cleared targets (zfresh is a constant there) and compiles none of them.  Visits, coverage iterations and
        // scan-line items never compare against W, H or the band in any kernel: a polygon's box is clamped to the frame
        // by the vertex stage and to the wave's region here (bx0..bx1, by0..by1, pair_box), so coverage stays inside
        // the tile, and the keys are LDS.
        static_assert(!INTERIOR || GROUP, "an interior kernel reads no previous depth");
        // this lane's key in block column 0 (block row 0; block row 1 follows SH ? 8 rows : NBX blocks later)
        const uint32_t key_lane = SH ? shared_key_slot((uint32_t)lx, (uint32_t)ly) : lane;
        // ---- initial keys -------------------------------------------------------------------
        if (SH) {
            // the waves initialise the tile's blocks between them
            for (int b = (int)wave; b < NBX * NBY; b += TILE_WAVES) {
                uint32_t zb = TR_F32_MIN_BITS;
                if (!zfresh) {
                    const int32_t px = qx0 + (b % NBX) * 8 + lx, py = qy0 + (b / NBX) * 8 + ly;
                    if (px < W && py >= band_y0 && py < band_y1)
                        zb = __float_as_uint(gload(depth + ((size_t)py * W + px)));
                }
                wkey[shared_key_slot((uint32_t)((b % NBX) * 8 + lx), (uint32_t)((b / NBX) * 8 + ly))] =
                    make_uint2(PREV_TAG, depth_order_bits(__uint_as_float(zb)));
            }
        } else {
    #pragma unroll
            for (int b = 0; b < NBX * NBY; b++) {
                uint32_t zb = TR_F32_MIN_BITS;
                if (!zfresh) {
                    const int32_t px = qx0 + (b % NBX) * 8 + lx, py = qy0 + (b / NBX) * 8 + ly;
                    if (px < W && py >= band_y0 && py < band_y1)
                        zb = __float_as_uint(gload(depth + ((size_t)py * W + px)));
                }
                wkey[(b << 6) + (lane ^ key_row_swizzle((uint32_t)((int32_t)wave * QUAD + (b % NBX) * 8)))] = make_uint2(zb, 0u);
            }
        }

        // ---- coverage + depth resolve ---------------------------------------------------------
        // The bin (n records of P 16-byte pieces, contiguous) is copied to LDS by all 256 threads,
        // NMAX records at a time.  Each wave then takes 64 records at a time into registers (lane l
        // holds the raster part of record l), ballots which of them touch its quadrant and walks
        // those, broadcasting a record to the scalar registers with v_readlane: no memory access at
        // all per polygon.
        for (uint32_t c0 = 0; c0 < n; c0 += NMAX) {
            const uint32_t m = min((uint32_t)NMAX, n - c0);
            if (c0 != 0u) __syncthreads();  // every wave is done with the previous chunk
            for (uint32_t q = tid; q < m * P; q += (uint32_t)TILE_THREADS) s_rec[q] = gload(bin + ((size_t)c0 * P + q));
            __syncthreads();
            if (stamps && c0 == 0u) t_staged = wall_clock64();

            // column mode: every wave takes all m records, 64 per round; shared mode: record jj belongs to
            // wave jj mod TILE_WAVES, a round covers 64 * TILE_WAVES records
            for (uint32_t j0 = 0; j0 < m; j0 += SH ? 64u * (uint32_t)TILE_WAVES : 64u) {
                const uint32_t jj = SH ? j0 + lane * (uint32_t)TILE_WAVES + wave : j0 + lane;
                uint4 r0 = make_uint4(1u, 0u, 0u, 0u), r1 = make_uint4(0, 0, 0, 0), r2 = r1;  // (no record: an empty box)
                if (jj < m) {
                    r0 = s_rec[jj * P + 0];
                    r1 = s_rec[jj * P + 1];
                    r2 = s_rec[jj * P + 2];
                }
                // piece 0: the polygon's clamped box and what k_setup found out about it inside THIS tile
                // (pair_masks, tr_shaders.h): the cells of a small pair, the block columns of a large one
                const int32_t rbx0 = (int32_t)(r0.x & 0xFFFFu), rbx1 = (int32_t)(r0.x >> 16);
                const int32_t rby0 = (int32_t)(r0.y & 0xFFFFu), rby1 = (int32_t)(r0.y >> 16);
                const PairBox pb = pair_box(rbx0, rbx1, rby0, rby1, tile_x0, qy0);
                const bool some = rbx0 <= rbx1;
                // Shared form: a SMALL polygon -- its box inside the tile at most SCAN_MAX_CHUNKS 8-pixel chunks
                // wide -- is not visited by a whole wave (135 instructions of broadcast and prologue for a
                // polygon of a hundred pixels, then 128 pixel slots per step of which a third lie in its
                // box): the live cells of its box (one row x one chunk each) become ITEMS, and the items of
                // all the tile's small polygons are dealt to the lanes of all its waves (below).
                const bool small = SH && SCAN_ITEMS && some && pb.nch <= SCAN_MAX_CHUNKS;
                const uint32_t items = small ? (uint32_t)(__popc(r0.z) + __popc(r0.w)) : 0u;
                // block columns of this wave's region (bit i = column pair i: block rows 0 / 1) with a live
                // block: what a visit iterates over
                uint32_t lmask = (some && !small) ? pair_block_columns(r0.z, r0.w, SHARED && SCAN_ITEMS, pb, tile_x0) : 0u;
                if (!SH) lmask = (lmask >> (NBX * wave)) & ((1u << NBX) - 1u);
                // The polygon's part of to_barycentric_coord (scene.rs:178-187).  Orientation is normalised so
                // that cross.z > 0: negating a0, a1, b0, b1 flips the sign of cross.x and cross.y exactly, and
                // dividing them by -cross.z (reciprocal -y) gives bit-identical quotients, so one branch-free form
                // of the inside test serves both windings.  cross.z is formed for the 64 records of this round at
                // once (lane l = record l); a visit takes it and the block columns from lane l (two v_readlane) and
                // everything else with scalar loads of the record in the tile's bin -- a few hundred bytes per tile,
                // resident in the scalar cache -- negating by the sign bit (bit l of `flip`) where cross.z < 0.
                // (Only the comparisons here use the normalised form: shading reads the raw fields, whose zero
                // signs its quotients keep.)
                const float lcz_raw = __uint_as_float(r1.z) * __uint_as_float(r2.y) - __uint_as_float(r2.x) * __uint_as_float(r1.w);
                const unsigned long long flip = __ballot(lcz_raw < 0.0f);
                const float lcz = lcz_raw < 0.0f ? -lcz_raw : lcz_raw;
                unsigned long long todo = (TR_DBG_SKIP & 4) ? 0ull : __ballot(lmask != 0u);
                while (todo) {
                    const uint32_t l = (uint32_t)__builtin_ctzll(todo);
                    todo &= todo - 1ull;
                    const uint32_t slot1 = SH ? c0 + j0 + l * (uint32_t)TILE_WAVES + wave + 1u : c0 + j0 + l + 1u;
                    const constant_ptr<uint32_t> rec = bin_s + (slot1 - 1u) * (uint32_t)(4 * P);  // (word 4 i + c = piece i, component c)
                    const uint4 g0 = make_uint4(rec[0], rec[1], 0u, 0u), g1 = make_uint4(rec[4], rec[5], rec[6], rec[7]);
                    const uint4 g2 = make_uint4(rec[8], rec[9], rec[10], rec[11]), g3 = make_uint4(rec[12], rec[13], 0u, 0u);
                    const uint32_t gry = rec[4 * P - 1];
                    const uint32_t sgn = ((uint32_t)(flip >> l) & 1u) << 31;
                    const uint32_t boxx = g0.x, boxy = g0.y;
                    const int32_t bx0 = imax((int32_t)(boxx & 0xFFFFu), qx0), bx1 = imin((int32_t)(boxx >> 16), qx0 + QUAD - 1);
                    const int32_t by0 = imax((int32_t)(boxy & 0xFFFFu), qy0), by1 = imin((int32_t)(boxy >> 16), qy0 + TILE_H - 1);
                    const int32_t x0 = (int32_t)g1.x, y0 = (int32_t)g1.y;
                    const float z0 = __uint_as_float(g2.z), z1 = __uint_as_float(g2.w);
                    const float z2 = __uint_as_float(g3.x);
                    const uint32_t id = g3.y;
                    uint32_t cols = (uint32_t)bcast(lmask, l);
                    Edge2T<V2> e;
                    e.a0 = splat2v<V2>(__uint_as_float(g1.z ^ sgn));
                    e.a1 = splat2v<V2>(__uint_as_float(g2.x ^ sgn));
                    e.b0 = splat2v<V2>(__uint_as_float(g1.w ^ sgn));
                    e.b1 = splat2v<V2>(__uint_as_float(g2.y ^ sgn));
                    const float cz = __int_as_float(bcast(__float_as_uint(lcz), l));
                    e.cz = splat2v<V2>(cz);
                    e.y = splat2v<V2>(__uint_as_float(gry ^ sgn));
                    // this lane's two pixels: (px, pya) in block row 0 and (px, pyb) in block row 1
                    const int32_t pya = qy0 + ly, pyb = qy0 + 8 + ly;
                    const V2 b2 = mk2v<V2>((float)isub(y0, pya), (float)isub(y0, pyb));
                    // the inside test (scene.rs:245-247 on to_barycentric_coord's cross products, divided
                    // by cross.z > 0): cross.x >= 0, cross.y >= 0, cross.x + cross.y <= cross.z.  The last is
                    // taken as cross.z - (cross.x + cross.y) >= 0 (same truth value: a difference of two
                    // floats has the sign of the exact difference) so that one three-way minimum and one
                    // compare decide a pixel; a row outside the clamped box gets -inf for cross.z.
                    const bool rowa = pya >= by0 && pya <= by1, rowb = pyb >= by0 && pyb <= by1;
                    const V2 czp = mk2v<V2>(rowa ? cz : -__builtin_inff(), rowb ? cz : -__builtin_inff());
                    while (cols) {
                        const int32_t ib = (int32_t)__builtin_ctz(cols);
                        cols &= cols - 1u;
                        // the two pixels' current keys, requested before the arithmetic that decides
                        // whether they are needed (LDS latency hidden inside the wave)
                        uint2 *slot_a = SH ? wkey + (key_lane ^ ((uint32_t)ib << 3))
                                           : wkey + (((uint32_t)ib << 6) + (lane ^ key_row_swizzle((uint32_t)((int32_t)wave * QUAD + ib * 8))));
                        uint2 *slot_b = slot_a + (SH ? 8 * TILE_W : NBX << 6);
                        const uint2 cur_a = *slot_a, cur_b = *slot_b;
                        const int32_t px = qx0 + ib * 8 + lx;
                        const bool inx = (uint32_t)isub(px, bx0) <= (uint32_t)isub(bx1, bx0);
                        V2 cx, cy;
                        edge_cross2(e, splat2v<V2>((float)isub(x0, px)), b2, cx, cy);
                        const V2 rest = czp - (cx + cy);
                        const bool hita = inx && __builtin_fminf(__builtin_fminf(cx.x, cy.x), rest.x) >= 0.0f;
                        const bool hitb = inx && __builtin_fminf(__builtin_fminf(cx.y, cy.y), rest.y) >= 0.0f;
                        if (SH) {
                            if (hita || hitb) {
                                // shared keys: the candidate (depth order bits, tie-break word) against what the
                                // pixel holds now -- a plain read, possibly stale, but keys only grow, so a
                                // candidate that does not beat it can never win -- then one atomic maximum
                                const Bary2T<V2> bar = barycentric2_for_compare(cx, cy, e);
                                const V2 z = dot3_2(bar.x, bar.y, bar.z, splat2v<V2>(z0), splat2v<V2>(z1), splat2v<V2>(z2));
                                const uint32_t tag = (((SHARED_MAX_POLYGONS - 1u) - id) << 12) | slot1;
                                const unsigned long long ka = ((unsigned long long)depth_order_bits(z.x) << 32) | tag;
                                const unsigned long long kb = ((unsigned long long)depth_order_bits(z.y) << 32) | tag;
                                const unsigned long long ca_ = ((unsigned long long)cur_a.y << 32) | cur_a.x;
                                const unsigned long long cb_ = ((unsigned long long)cur_b.y << 32) | cur_b.x;
                                if (hita && ka > ca_)
                                    __hip_atomic_fetch_max(reinterpret_cast<unsigned long long *>(slot_a), ka, __ATOMIC_RELAXED,
                                                           __HIP_MEMORY_SCOPE_WORKGROUP);
                                if (hitb && kb > cb_)
                                    __hip_atomic_fetch_max(reinterpret_cast<unsigned long long *>(slot_b), kb, __ATOMIC_RELAXED,
                                                           __HIP_MEMORY_SCOPE_WORKGROUP);
                            }
                        } else if (hita || hitb) {
                            // depth of both fragments; only compared here (the survivor's stored z is
                            // recomputed with exact zero signs when it is shaded)
                            const Bary2T<V2> bar = barycentric2_for_compare(cx, cy, e);
                            const V2 z = dot3_2(bar.x, bar.y, bar.z, splat2v<V2>(z0), splat2v<V2>(z1), splat2v<V2>(z2));
                            // both comparisons first, branch-free, so that the two key reads above are
                            // consumed together after the arithmetic; equal depths (shared vertices and
                            // edges, or the buffer's previous content) are the rare divergent path
                            const float zca = __uint_as_float(cur_a.x), zcb = __uint_as_float(cur_b.x);
                            bool wina = hita && z.x > zca, winb = hitb && z.y > zcb;
                            const bool tiea = hita && z.x == zca, tieb = hitb && z.y == zcb;
                            if (tiea || tieb) {
                                // equal depth: the buffer's previous content beats a colour fragment
                                // (`z <= zbuf` rejects) and loses to a depth fragment (`z >= shadow`
                                // accepts); between two fragments of this pass the polygon index decides
    #pragma unroll
                                for (int h = 0; h < 2; h++) {
                                    if (!(h == 0 ? tiea : tieb)) continue;
                                    const uint32_t cs = h == 0 ? cur_a.y : cur_b.y;
                                    bool w = DEPTH;
                                    if (cs != 0u) {
                                        const uint32_t cur_id = resident ? s_rec[(cs - 1u) * P + 3].y
                                                                         : gload(bin + ((size_t)(cs - 1u) * P + 3)).y;
                                        w = DEPTH ? id > cur_id : id < cur_id;
                                    }
                                    if (h == 0) wina = w; else winb = w;
                                }
                            }
                            if (wina) *slot_a = make_uint2(__float_as_uint(z.x), slot1);
                            if (winb) *slot_b = make_uint2(__float_as_uint(z.y), slot1);
                        }
                    }
                }

                if (SH && SCAN_ITEMS) {
                    // ---- scan-line items of the round's small polygons --------------------------------
                    // Items are numbered over the whole workgroup (thread order), 64 of them make a pass and
                    // pass p belongs to wave p mod TILE_WAVES: every wave gets the same share wherever the
                    // polygons sit in the bin.  A lane finds the record its item belongs to by a binary search
                    // in the running sums and reads the record from LDS itself -- no broadcast at all -- then
                    // tests the item's 8 pixels two at a time: (x, x + 1) in packed arithmetic with exactly
                    // the operations of the visit above (scene.rs:178-187, 245-247, shader.rs:174).
                    uint32_t incl = items;
    #pragma unroll
                    for (int d = 1; d < 64; d <<= 1) {
                        const uint32_t up = (uint32_t)__shfl_up((int)incl, d, 64);
                        if ((int)lane >= d) incl += up;
                    }
                    if (lane == 63u) s_wtot[wave] = incl;
                    __syncthreads();  // (also: every wave is done with the previous round's sums)
                    uint32_t before = 0u, total = 0u;
    #pragma unroll
                    for (int w = 0; w < TILE_WAVES; w++) {
                        const uint32_t t = s_wtot[w];
                        before += (uint32_t)w < wave ? t : 0u;
                        total += t;
                    }
                    total = (uint32_t)__builtin_amdgcn_readfirstlane((int)total);
                    s_incl[tid] = before + incl;
                    __syncthreads();
                    for (uint32_t pass = wave; !(TR_DBG_SKIP & 2) && pass * 64u < total; pass += (uint32_t)TILE_WAVES) {
                        const uint32_t item = pass * 64u + lane;
                        const bool act = item < total;
                        // owner = the first thread whose running sum exceeds the item's number
                        uint32_t lo = 0u, hi = (uint32_t)TILE_THREADS - 1u;
    #pragma unroll
                        for (int i = 0; i < 6 + (TILE_WAVES == 4 ? 2 : TILE_WAVES == 8 ? 3 : 4); i++) {
                            const uint32_t mid = (lo + hi) >> 1;
                            if (s_incl[mid] > item)
                                hi = mid;
                            else
                                lo = mid + 1u;
                        }
                        const uint32_t q = item - (lo ? s_incl[lo - 1u] : 0u);
                        // thread lo = lane lo & 63 of wave lo >> 6 holds record j0 + lane * TILE_WAVES + wave
                        const uint32_t rec = act ? j0 + (lo & 63u) * (uint32_t)TILE_WAVES + (lo >> 6) : 0u;
                        const uint4 *const R = s_rec + mul24(rec, (uint32_t)P);
                        const uint4 q0 = R[0], q1 = R[1], q2 = R[2];
                        const uint2 q3 = *reinterpret_cast<const uint2 *>(R + 3);
                        const float ryv = __uint_as_float(R[P - 1].w);
                        // the item = the q-th live cell of the pair's mask: row `cell / 4` of the box inside the
                        // tile, chunk `cell % 4` = pixels xs .. xs + 7 of that row (xs even)
                        const PairBox ib = pair_box((int32_t)(q0.x & 0xFFFFu), (int32_t)(q0.x >> 16), (int32_t)(q0.y & 0xFFFFu),
                                                    (int32_t)(q0.y >> 16), tile_x0, qy0);
                        uint32_t cell;
                        {
                            const uint32_t nlo = (uint32_t)__popc(q0.z);
                            const bool upper = q >= nlo;
                            uint32_t w = upper ? q0.w : q0.z, k = upper ? q - nlo : q;
                            cell = upper ? 32u : 0u;
    #pragma unroll
                            for (int sh = 16; sh >= 1; sh >>= 1) {
                                const uint32_t below = (uint32_t)__popc(w & ((1u << sh) - 1u));
                                const bool up = k >= below;
                                k -= up ? below : 0u;
                                w = up ? w >> sh : w;
                                cell += up ? (uint32_t)sh : 0u;
                            }
                        }
                        const int32_t py = ib.ay0 + (int32_t)(cell >> 2), xs = ib.xs + 8 * (int32_t)(cell & 3u);
                        // pixels of the chunk inside the box, as a bit mask (bit i = pixel xs + i)
                        const uint32_t first = (uint32_t)imax(isub(ib.ax0, xs), 0) & 7u, last = (uint32_t)imin(isub(ib.ax1, xs), 7) & 7u;  // (in 0..7 for a live item)
                        const uint32_t inmask = act ? (2u << last) - (1u << first) : 0u;
                        // the polygon's constants, orientation-normalised as above
                        float a0 = __uint_as_float(q1.z), b0 = __uint_as_float(q1.w);
                        float a1 = __uint_as_float(q2.x), b1 = __uint_as_float(q2.y);
                        float cz = a0 * b1 - a1 * b0, yv = ryv;
                        if (cz < 0.0f) {
                            a0 = -a0; a1 = -a1; b0 = -b0; b1 = -b1;
                            cz = -cz;
                            yv = -yv;
                        }
                        const int32_t x0 = (int32_t)q1.x;
                        const float bf = (float)isub((int32_t)q1.y, py);
                        const V2 a1b = splat2v<V2>(a1 * bf), a0b = splat2v<V2>(a0 * bf);  // e.a1 * b2, e.a0 * b2 of edge_cross2
                        Edge2T<V2> e;
                        e.cz = splat2v<V2>(cz);
                        e.y = splat2v<V2>(yv);
                        const V2 z0 = splat2v<V2>(__uint_as_float(q2.z)), z1 = splat2v<V2>(__uint_as_float(q2.w));
                        const V2 z2 = splat2v<V2>(__uint_as_float(q3.x));
                        const uint32_t tag = (((SHARED_MAX_POLYGONS - 1u) - q3.y) << 12) | (c0 + rec + 1u);
                        const uint32_t yrel = (uint32_t)isub(py, qy0) & (uint32_t)(TILE_H - 1);
                        const uint32_t xrel = (uint32_t)isub(xs, qx0) & (uint32_t)(TILE_W - 2);
                        const uint32_t key_row = yrel * (uint32_t)TILE_W, key_sw = (yrel & 7u) << 3;
    #pragma unroll
                        for (int k = 0; k < 4; k++) {
                            const uint32_t kx = (xrel + 2u * k) & (uint32_t)(TILE_W - 1);  // (a chunk may start up to 6 pixels from the tile's end: wraps, masked out)
                            uint4 *const slot = reinterpret_cast<uint4 *>(wkey + (key_row + (kx ^ key_sw)));
                            const uint4 cur = *slot;
                            const int32_t px = xs + 2 * k;
                            const V2 a2 = mk2v<V2>((float)isub(x0, px), (float)isub(x0, px + 1));
                            const V2 cx = a1b - a2 * splat2v<V2>(b1), cy = a2 * splat2v<V2>(b0) - a0b;
                            const V2 rest = e.cz - (cx + cy);
                            const bool hita = ((inmask >> (2 * k)) & 1u) && __builtin_fminf(__builtin_fminf(cx.x, cy.x), rest.x) >= 0.0f;
                            const bool hitb = ((inmask >> (2 * k + 1)) & 1u) && __builtin_fminf(__builtin_fminf(cx.y, cy.y), rest.y) >= 0.0f;
                            if (hita || hitb) {
                                const Bary2T<V2> bar = barycentric2_for_compare(cx, cy, e);
                                const V2 z = dot3_2(bar.x, bar.y, bar.z, z0, z1, z2);
                                const unsigned long long ka = ((unsigned long long)depth_order_bits(z.x) << 32) | tag;
                                const unsigned long long kb = ((unsigned long long)depth_order_bits(z.y) << 32) | tag;
                                const unsigned long long ca_ = ((unsigned long long)cur.y << 32) | cur.x;
                                const unsigned long long cb_ = ((unsigned long long)cur.w << 32) | cur.z;
                                if (hita && ka > ca_)
                                    __hip_atomic_fetch_max(reinterpret_cast<unsigned long long *>(slot), ka, __ATOMIC_RELAXED,
                                                           __HIP_MEMORY_SCOPE_WORKGROUP);
                                if (hitb && kb > cb_)
                                    __hip_atomic_fetch_max(reinterpret_cast<unsigned long long *>(slot) + 1, kb, __ATOMIC_RELAXED,
                                                           __HIP_MEMORY_SCOPE_WORKGROUP);
                            }
                        }
                    }
                }
            }
        }

    };
    if (shared_tile)
        resolve(std::bool_constant<SHARED>{});
    else
        resolve(std::false_type{});

    uint64_t t_covered = 0;
    if (stamps) t_covered = wall_clock64();

    // ---- shade the survivors and stream the tile out ------------------------------------------
    // Lanes are row-major here: lane = x within a 32-pixel row; a step covers four rows, each
    // lane carrying the two pixels (x, 4s + half) and (x, 4s + 2 + half) through packed
    // arithmetic.  Depth goes out straight from registers as whole 128-byte lines and colour is
    // packed to dwords with two lane permutes; the vertical flip of get_frame_buffer
    // (scene.rs:92-97) is folded into the colour address.  Lanes without a survivor run the same
    // loads on record 0 and discard the result, so the code is branch-free inside a step.
    // Addresses are a per-wave base (scalar registers) plus a 32-bit lane offset built with 24-bit
    // multiplies: 64-bit and 32 x 32 multiplies run at quarter rate and were a third of this
    // phase's vector-ALU time.
    if (SHARED || TILE_WAVES != TILE_W / STRIP) __syncthreads();  // a strip may hold pixels other waves resolved
    const int32_t hx = (int32_t)(lane & 31u), hrow = (int32_t)(lane >> 5);
    const uint32_t half_base = lane & 32u;
    const int32_t strip_x = (int32_t)(wave / (uint32_t)WAVES_PER_STRIP) * STRIP;  // within the tile
    const int32_t strip_y = (int32_t)(wave % (uint32_t)WAVES_PER_STRIP) * STRIP_ROWS;
    const int32_t sx0 = tile_x0 + strip_x, sy0 = qy0 + strip_y;
    const int32_t px = sx0 + hx;
    constexpr int NSTEP = STRIP_ROWS / 4;
    // strip origins: depth/winner at row sy0, colour at the strip's last row (lowest address of
    // the flipped image), so every lane offset is non-negative.  Rows outside the frame or the
    // band give addresses that are formed but never used.
    float *const depth_strip = depth + ((int64_t)sy0 * W + sx0);
    uint32_t *const winner_strip = (!GROUP && a.winner) ? a.winner + ((int64_t)sy0 * W + sx0) : nullptr;
    uint8_t *const fb_strip = DEPTH ? nullptr : fb + ((int64_t)(H - sy0 - STRIP_ROWS) * W + sx0) * 3;
    const uint32_t Wu = (uint32_t)W, W3 = 3u * (uint32_t)W;
    // (INTERIOR: px < tile_x0 + TILE_W <= ntx * TILE_W = W)
    const bool col_live = INTERIOR || px < W;
    // What a step's keys and stores need of the lane is the same in every step; only the step's first row r0 (even,
    // uniform) moves them, and it moves them by scalars:
    //   key slot   key_slot(x, strip_y + r0 + hrow) = (key_slot(x, hrow) ^ ((r0' & 7) << 3)) + ((r0' >> 3) * NBX << 6),
    //              r0' = strip_y + r0 -- the rows of an 8x8 block sit in slot bits 3..5 (r0' even: it and hrow share no bit),
    //              the block row above bit 6;
    //   depth      row r0 + hrow at depth_strip + r0 * W (scalar) + (hrow * W + hx);
    //   colour     rows r0 / r0 + 1 at fb_strip + (STRIP_ROWS - 2 - r0) * 3W (scalar) + ((1 - hrow) * 3W + 3 hx / 4 hx).
    // So the step loop forms no address arithmetic of its own beyond one XOR per key.
    const uint32_t key_lane = key_slot<QUAD_COLUMN>((uint32_t)strip_x + (uint32_t)hx, (uint32_t)hrow);
    const uint32_t zlane = mul24((uint32_t)hrow, Wu) + (uint32_t)hx;
    const uint32_t clane = mul24(1u - (uint32_t)hrow, W3);
    // the dword form of the colour row: dword j of the 96-byte row = bytes 4j..4j+3 = pixel p0 = 4j/3 from byte (4j)%3 on,
    // topped up from pixel p0+1 -- the two permutes' byte addresses (ds_bpermute) and shifts of this lane
    const uint32_t cj = (uint32_t)hx, cp0 = (4u * cj) / 3u, co = (4u * cj) % 3u;
    const int32_t perm0 = (int32_t)((half_base + (cp0 & 31u)) << 2), perm1 = (int32_t)((half_base + ((cp0 + 1u) & 31u)) << 2);
    const uint32_t csh0 = 8u * co, csh1 = 24u - 8u * co;
    // (INTERIOR: the strip's 96 bytes end at 3 (sx0 + STRIP) <= 3 W: a lane constant)
    const bool cdw_live = cj < 24u && (INTERIOR || (sx0 * 3 + (int32_t)(4u * cj)) < W * 3);

    // Reads a pixel's key and returns the bin slot + 1 of its survivor (0: none): pixel (hx, r0 + hrow) of the strip
    // (zbits: the f32 bits of the depth the resolve compared for that pixel -- what a depth pass stores, below)
    auto survivor_slot = [&](uint32_t r0, uint32_t &zbits) -> uint32_t {
        if (SHARED && shared_tile) {
            // tie-break word: low 12 bits = bin slot + 1 of a fragment, 0xFFF / 0 = the buffer's old content
            const uint2 key = s_key[shared_key_slot((uint32_t)strip_x + (uint32_t)hx, (uint32_t)strip_y + r0 + (uint32_t)hrow)];
            const uint32_t f = key.x & 0xFFFu;
            zbits = (key.y & 0x80000000u) ? key.y ^ 0x80000000u : ~key.y;  // (depth_order_bits undone; both zeros read +0)
            return (f == 0xFFFu) ? 0u : f;
        }
        const uint32_t ry = (uint32_t)strip_y + r0;
        const uint32_t slot = (key_lane ^ ((ry & 7u) << 3)) + (((ry >> 3) * (uint32_t)(QUAD_COLUMN / 8)) << 6);
        // (the whole 8-byte key: 64 lanes x 8 bytes in a row are conflict-free as ds_read_b64, the upper dwords alone as
        // ds_read_b32 are a two-way bank conflict)
#if TR_KEY_B64
        const uint2 key = s_key[slot];
        uint32_t keep = key.x;
        asm volatile("" : "+v"(keep));   // (keeps the compiler from narrowing the read again)
        zbits = keep;
        return key.y;
#else
        zbits = 0u;
        return s_key[slot].y;
#endif
    };
    // Two pixels of a lane through the fragment stage, each against its own polygon: pixel u at (pxs[u], pys[u]),
    // survivor in bin slot wslot[u] if won[u] -- for records in LDS the key's slot + 1 as it was read (no select: a lane
    // without a survivor reads the 96 bytes in front of record 0, or record slot + 1 - 1 of a pixel outside the band, and
    // discards the result), for records in global memory the slot itself (record 0 for a lane without a survivor).
    // So the code is branch-free.  RESIDENT: the bin's records are in LDS (nearly always);
    // PAIR: the two-pixel closures (tr_shaders.h) -- returns true when a surviving pixel left their guarded
    // range anywhere in the wave (the caller then runs the step again with the plain closures; keeping those
    // out of the fast loop's body matters: inline, as the fallback of each step, their registers were live
    // across the fast path and cost 5-9 % although they almost never ran).
    auto shade_two = [&](auto in_lds, auto pair_tag, const int32_t (&pxs)[2], const int32_t (&pys)[2], const bool (&won)[2],
                         const uint32_t (&wslot)[2], float (&zout)[2], uint32_t (&rgb)[2], uint32_t (&tri)[2]) -> bool {
        constexpr bool RESIDENT = decltype(in_lds)::value;
        constexpr bool PAIR = decltype(pair_tag)::value;
        bool redo = false;
        // The two survivors' records.  Pieces 1..TOP-1 (raster part, uv and, for the 6-piece record,
        // everything else) are taken for both pixels at once; the darboux record's further 16
        // varyings per pixel are fetched when that pixel's closure runs, one pixel after the other,
        // so that 32 fewer registers are live (123 -> under 96: a fifth wave per SIMD).
        constexpr int TOP = P < 6 ? P : 6;
        uint4 qa[TOP], qb[TOP];
        const uint4 *const ra = RESIDENT ? s_rec + ((int32_t)mul24(wslot[0], (uint32_t)P) - P) : bin + (size_t)wslot[0] * P;
        const uint4 *const rb = RESIDENT ? s_rec + ((int32_t)mul24(wslot[1], (uint32_t)P) - P) : bin + (size_t)wslot[1] * P;
#pragma unroll
        for (int i = 1; i < TOP; i++) {
            qa[i] = RESIDENT ? ra[i] : gload(ra + i);
            qb[i] = RESIDENT ? rb[i] : gload(rb + i);
        }
        const uint32_t rya = P > TOP ? (RESIDENT ? ra[P - 1].w : gload(ra + (P - 1)).w) : qa[TOP - 1].w;
        const uint32_t ryb = P > TOP ? (RESIDENT ? rb[P - 1].w : gload(rb + (P - 1)).w) : qb[TOP - 1].w;
        // to_barycentric_coord for both pixels (each against its own polygon)
        Edge2T<V2> e;
        e.a0 = mk2v<V2>(__uint_as_float(qa[1].z), __uint_as_float(qb[1].z));
        e.a1 = mk2v<V2>(__uint_as_float(qa[2].x), __uint_as_float(qb[2].x));
        e.b0 = mk2v<V2>(__uint_as_float(qa[1].w), __uint_as_float(qb[1].w));
        e.b1 = mk2v<V2>(__uint_as_float(qa[2].y), __uint_as_float(qb[2].y));
        e.cz = e.a0 * e.b1 - e.a1 * e.b0;
        e.y = mk2v<V2>(__uint_as_float(rya), __uint_as_float(ryb));
        const V2 a2 = mk2v<V2>((float)isub((int32_t)qa[1].x, pxs[0]), (float)isub((int32_t)qb[1].x, pxs[1]));
        const V2 b2 = mk2v<V2>((float)isub((int32_t)qa[1].y, pys[0]), (float)isub((int32_t)qb[1].y, pys[1]));
        V2 cx, cy;
        edge_cross2(e, a2, b2, cx, cy);
        const Bary2T<V2> bar = barycentric2(cx, cy, e);
        const V2 z = dot3_2(bar.x, bar.y, bar.z, mk2v<V2>(__uint_as_float(qa[2].z), __uint_as_float(qb[2].z)),
                            mk2v<V2>(__uint_as_float(qa[2].w), __uint_as_float(qb[2].w)),
                            mk2v<V2>(__uint_as_float(qa[3].x), __uint_as_float(qb[3].x)));
        uint32_t ca = 0u, cb = 0u, ea = 0u, eb = 0u;
        if (!DEPTH && st_c) {   // (a depth-only repeat of a colour pass: the z, no closure)
            // uv = vertex_uvs * bar (2x3 gemv), both pixels
            V2 uu = mk2v<V2>(__uint_as_float(qa[3].z), __uint_as_float(qb[3].z)) * bar.x;
            V2 vv = mk2v<V2>(__uint_as_float(qa[3].w), __uint_as_float(qb[3].w)) * bar.x;
            uu = mk2v<V2>(__uint_as_float(qa[4].x), __uint_as_float(qb[4].x)) * bar.y + uu;
            vv = mk2v<V2>(__uint_as_float(qa[4].y), __uint_as_float(qb[4].y)) * bar.y + vv;
            uu = mk2v<V2>(__uint_as_float(qa[4].z), __uint_as_float(qb[4].z)) * bar.z + uu;
            vv = mk2v<V2>(__uint_as_float(qa[4].w), __uint_as_float(qb[4].w)) * bar.z + vv;
            if (FS == FS_LIT) {
                // the frame's lit texel image (k_lit): the closure has run for this texel already
                uint32_t unused1, unused2;
                vec3 unused3;
                fetch_texels<FS>(tex, uu.x, vv.x, ea, ca, unused1, unused2, unused3);
                fetch_texels<FS>(tex, uu.y, vv.y, eb, cb, unused1, unused2, unused3);
            } else if (FS == FS_DEFAULT || FS == FS_PHONG) {
                // shader.rs:318-333 / 386-401 for both pixels at once: texel, diffuse term,
                // color_blend(c, 0, t) = (t * c + (1 - t) * 0.0) as u8 per channel
                uint32_t ta, tb, unused1, unused2;
                vec3 unused3;
                fetch_texels<FS>(tex, uu.x, vv.x, ea, ta, unused1, unused2, unused3);
                fetch_texels<FS>(tex, uu.y, vv.y, eb, tb, unused1, unused2, unused3);
                V2 t = mk2v<V2>(__uint_as_float(qa[5].x), __uint_as_float(qb[5].x));
                if (FS == FS_PHONG)
                    t = dot3_2(bar.x, bar.y, bar.z, t, mk2v<V2>(__uint_as_float(qa[5].y), __uint_as_float(qb[5].y)),
                               mk2v<V2>(__uint_as_float(qa[5].z), __uint_as_float(qb[5].z)));
#if TR_BLEND_FAST
                t = mk2v<V2>(blend_weight(t.x), blend_weight(t.y));  // (blend_black, tr_math.h: the (1 - t) * 0.0 term as a select)
#else
                const V2 k = (splat2v<V2>(1.0f) - t) * splat2v<V2>(0.0f);
#endif
#pragma unroll
                for (int ch = 0; ch < 3; ch++) {
#if TR_BLEND_FAST
                    const V2 v = t * mk2v<V2>((float)((ta >> (8 * ch)) & 0xFFu), (float)((tb >> (8 * ch)) & 0xFFu));
#else
                    const V2 v = t * mk2v<V2>((float)((ta >> (8 * ch)) & 0xFFu), (float)((tb >> (8 * ch)) & 0xFFu)) + k;
#endif
                    ca = pack_u8(v.x, (uint32_t)ch, ca);   // (`as u8` and the byte's place in one step, tr_math.h)
                    cb = pack_u8(v.y, (uint32_t)ch, cb);
                }
            } else {
                // one pixel's closure after the other's (interleaved they need twice the registers)
                auto closure = [&](const uint4 (&q)[TOP], const uint4 *rec, vec3 b, float u_, float v_, int32_t px_, int32_t py_,
                                   float z_, uint32_t &e_) {
                    float v[VARY_STRIDE];
                    v[0] = __uint_as_float(q[3].z); v[1] = __uint_as_float(q[3].w);
#pragma unroll
                    for (int i = 4; i < P; i++) {
                        const uint4 piece = i < TOP ? q[i] : (RESIDENT ? rec[i] : gload(rec + i));
                        v[4 * i - 14] = __uint_as_float(piece.x); v[4 * i - 13] = __uint_as_float(piece.y);
                        v[4 * i - 12] = __uint_as_float(piece.z); v[4 * i - 11] = __uint_as_float(piece.w);
                    }
                    return fragment_color<FS>(a.u, tex, v, b, u_, v_, (uint32_t)px_, (uint32_t)py_, z_, a.shadow,
                                              (uint32_t)W, (uint32_t)H, e_, a.sclean);
                };
                if constexpr (PAIR) {
                    // both pixels through the closure together in packed arithmetic with shared
                    // reciprocals (tr_shaders.h, fragment_color_pair); a step in which a surviving pixel's
                    // operands leave the range that form is proven on is run again with the plain
                    // closure (rare: exact zeros among the normalised components, a degenerate basis)
                    auto vary2 = [&](int k) -> f2 {
                        const int i = k < 2 ? 3 : (k + 14) / 4, c = k < 2 ? k + 2 : (k + 14) % 4;
                        const uint4 pa = i < TOP ? qa[i] : (RESIDENT ? ra[i] : gload(ra + i)), pb = i < TOP ? qb[i] : (RESIDENT ? rb[i] : gload(rb + i));
                        const uint32_t wa = c == 0 ? pa.x : c == 1 ? pa.y : c == 2 ? pa.z : pa.w;
                        const uint32_t wb = c == 0 ? pb.x : c == 1 ? pb.y : c == 2 ? pb.z : pb.w;
                        return mk2(__uint_as_float(wa), __uint_as_float(wb));
                    };
                    bool bad_a, bad_b;
                    vec3p barp;
                    // (the two-pixel closures are written for the packed type)
                    barp.x = to_f2(bar.x); barp.y = to_f2(bar.y); barp.z = to_f2(bar.z);
                    fragment_color_pair<FS>(a.u, tex, vary2, barp, to_f2(uu), to_f2(vv), ca, cb, ea, eb, bad_a, bad_b);
                    if (__any((bad_a && won[0]) || (bad_b && won[1]))) {
                        redo = true;
                        ea = eb = 0u;  // the second run reports this step's lookups
                    }
                } else {
                    ca = closure(qa, ra, make3(bar.x.x, bar.y.x, bar.z.x), uu.x, vv.x, pxs[0], pys[0], z.x, ea);
                    __builtin_amdgcn_sched_barrier(0);
                    cb = closure(qb, rb, make3(bar.x.y, bar.y.y, bar.z.y), uu.y, vv.y, pxs[1], pys[1], z.y, eb);
                }
            }
        }
        uint32_t err = 0u;
        if (won[0]) {
            zout[0] = z.x;
            rgb[0] = ca;
            tri[0] = qa[3].y;
            err |= ea;
        }
        if (won[1]) {
            zout[1] = z.y;
            rgb[1] = cb;
            tri[1] = qb[3].y;
            err |= eb;
        }
        if (err) {
            atomicOr(a.err, err);
            *a.alarm = 1u;
        }
        return redo;
    };

    // Pixel u of a lane's step to memory: row r0 + u * 2 + hrow of the strip (r0: the step's first row), `live` = inside
    // frame and band, `put` = its depth (and winner word) changes.  Depth goes out straight from registers as whole
    // 128-byte lines; colour is packed to dwords with two lane permutes and stored flipped (scene.rs:92-97 folded in).
    // aligned4: the frame's width is a multiple of 4 (TileArgs::aligned4), so a colour row is whole dwords (a uniform branch).
    auto store_pixel = [&](uint32_t r0, bool row_live, bool live, bool won, float zv, uint32_t rgbv,
                           uint32_t triv, bool with_winner) {
        uint8_t *const fb_row = DEPTH ? nullptr : fb_strip + (int64_t)((int32_t)(STRIP_ROWS - 2) - (int32_t)r0) * (int64_t)W3;
        if (!DEPTH && !fresh && live && !won && st_c) {
            // untouched pixel of an accumulate render: its colour may share a dword with a
            // touched neighbour, so fetch it
            const uint8_t *old = fb_row + (clane + 3u * (uint32_t)hx);
            rgbv = pack_rgb(gload(old), gload(old + 1), gload(old + 2));
        }
        // depth: only pixels that changed (or every live pixel of a fresh tile)
        const bool put = live && (won || zfresh);
        // (TileArgs::store: a cleared frame's colour pass may leave its depth on the chip -- nothing reads the z buffer
        // of such a frame unless a getter or an accumulating render asks, and then the pass is repeated for the depth alone)
        if (put && st_z) gstore(depth_strip + (int64_t)r0 * W + zlane, zv);
        if (!DEPTH && st_c) {
            if (winner_strip && put && with_winner) gstore(winner_strip + (int64_t)r0 * W + zlane, triv);
            if (INTERIOR || aligned4) {   // (INTERIOR: W is a multiple of TILE_W = 128 -- no byte-store arm)
                const uint32_t c0 = (uint32_t)__builtin_amdgcn_ds_bpermute(perm0, (int)rgbv);
                const uint32_t c1 = (uint32_t)__builtin_amdgcn_ds_bpermute(perm1, (int)rgbv);
                const uint32_t dw = (c0 >> csh0) | (c1 << csh1);
                if (cdw_live && row_live)
                    gstore(reinterpret_cast<uint32_t *>(fb_row + (clane + 4u * cj)), dw);
            } else if (put) {
                uint8_t *p = fb_row + (clane + 3u * (uint32_t)hx);
                gstore(p, (uint8_t)(rgbv & 0xFFu));
                gstore(p + 1, (uint8_t)((rgbv >> 8) & 0xFFu));
                gstore(p + 2, (uint8_t)((rgbv >> 16) & 0xFFu));
            }
        }
    };

    // ---- row-major form: lane = x within a 32-pixel row; a step covers four rows, each lane carrying the
    // two pixels (x, 4s + half) and (x, 4s + 2 + half) through the fragment stage and straight to memory.
    // Exists for bins that stay resident in LDS and for the rare larger ones, whose survivors' records come
    // from global memory -- a run-time choice inside the loop cost a dozen register moves per step where the
    // two paths merge.  Returns the steps to run again with the plain closures (every store of a step is
    // repeated, so the second run simply overwrites the first).
    auto shade_steps = [&](auto in_lds, auto pair_tag, uint32_t step_mask) -> uint32_t {
    constexpr bool RESIDENT = decltype(in_lds)::value;
    uint32_t redo = 0u;
#pragma unroll 1
    for (int32_t sstep = 0; sstep < NSTEP; sstep++) {
        if (!((step_mask >> sstep) & 1u)) continue;
        int32_t py[2];
        bool row_live[2], live[2], won[2];
        uint32_t wslot[2], zkey[2];
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const uint32_t r0 = (uint32_t)(sstep * 4 + u * 2);  // the pixel's row in the strip: r0 + hrow
            py[u] = sy0 + (int32_t)r0 + hrow;
            // (INTERIOR: tile rows ty_base .. ty_base + nty - 1 are rows band_y0 .. band_y1 - 1 exactly, and band_y1 <= H)
            row_live[u] = INTERIOR || (py[u] >= band_y0 && py[u] < band_y1);
            live[u] = col_live && row_live[u];
            const uint32_t s1 = survivor_slot(r0, zkey[u]);
            won[u] = live[u] && s1 != 0u;
            wslot[u] = RESIDENT ? s1 : (won[u] ? s1 - 1u : 0u);  // (shade_two)
        }
        uint32_t tri[2] = { NO_WINNER, NO_WINNER }, rgb[2] = { 0u, 0u };
        float zout[2] = { bits_f32(TR_F32_MIN_BITS), bits_f32(TR_F32_MIN_BITS) };
        // A depth pass (shader.rs:694-709, 832-847) stores the survivor's z and nothing else -- and the resolve has
        // computed exactly that value: the same polygon, the same pixel, the same operations (barycentric2_for_compare
        // differs from barycentric2 only in the SIGN of a zero quotient, which reaches the sum only when the sum is itself
        // a zero).  So the key's depth IS the stored depth unless it is a zero; a step with a zero among its survivors'
        // depths takes the fragment stage as before.  No record gather, no cross products, no quotients for the rest:
        // the depth pass of the reference's model at 4096^2 22.5 -> see profiles/r04_notes.md.
        bool from_keys = false;
        if (DEPTH && TR_DEPTH_FROM_KEYS && TR_KEY_B64) {
            from_keys = !__any((won[0] && (zkey[0] << 1) == 0u) || (won[1] && (zkey[1] << 1) == 0u));
            if (from_keys) {
                if (won[0]) zout[0] = __uint_as_float(zkey[0]);
                if (won[1]) zout[1] = __uint_as_float(zkey[1]);
            }
        }
        if (!(TR_DBG_SKIP & 1) && !from_keys && __any(won[0] || won[1])) {
            const int32_t pxs[2] = { px, px };
            if (shade_two(in_lds, pair_tag, pxs, py, won, wslot, zout, rgb, tri)) redo |= 1u << sstep;
        }
#pragma unroll
        for (int u = 0; u < 2; u++)
            store_pixel((uint32_t)(sstep * 4 + u * 2), row_live[u], live[u], won[u], zout[u], rgb[u], tri[u], true);
    }
    return redo;
    };

    constexpr uint32_t ALL_STEPS = (1u << NSTEP) - 1u;
    constexpr bool HAS_PAIR = has_pair_closure(FS);
    uint32_t redo;
    if (resident)
        redo = shade_steps(std::true_type{}, std::bool_constant<HAS_PAIR>{}, ALL_STEPS);
    else
        redo = shade_steps(std::false_type{}, std::bool_constant<HAS_PAIR>{}, ALL_STEPS);
    if (HAS_PAIR && redo != 0u) {
        if (resident)
            shade_steps(std::true_type{}, std::false_type{}, redo);
        else
            shade_steps(std::false_type{}, std::false_type{}, redo);
    }

    if (a.zclean && tid == 0u && st_z) a.zclean[tile] = 0u;
    if (!DEPTH && a.fbclean && tid == 0u && st_c) a.fbclean[tile] = 0u;

    if (stamps) {
        __syncthreads();
        if (tid == 0u) {
            stamps[8u * tile + 0u] = t_start;
            stamps[8u * tile + 1u] = wall_clock64();
            stamps[8u * tile + 2u] = n;
            stamps[8u * tile + 3u] = __smid();
            stamps[8u * tile + 4u] = t_staged;
            stamps[8u * tile + 5u] = t_covered;
        }
    }
}

// -----------------------------------------------------------------------------------------
// Small utility kernels
// -----------------------------------------------------------------------------------------

// Writes the f32::MIN of every colour-pass tile whose fast-clear flag is up and lowers the flag:
// run before anything reads the z buffer as plain memory (tr_scene_read_z_f32, get_z_buffer).
__global__ __launch_bounds__(256) void k_materialize_depth(float *zbuf, uint32_t *zclean, DevFrame frame)
{
    const uint32_t t = blockIdx.x;
    if (zclean[t] == 0u) return;
    const int32_t x0 = (int32_t)(t % frame.ntx) * TILE_W, y0 = (frame.ty_base + (int32_t)(t / frame.ntx)) * TILE_H;
    for (uint32_t p = threadIdx.x; p < (uint32_t)(TILE_W * TILE_H); p += 256u) {
        const int32_t y = y0 + (int32_t)(p / TILE_W), x = x0 + (int32_t)(p % TILE_W);
        if (x < (int32_t)frame.width && y >= frame.band_y0 && y < frame.band_y1)
            zbuf[(size_t)y * frame.width + x] = bits_f32(TR_F32_MIN_BITS);
    }
    __syncthreads();
    if (threadIdx.x == 0u) zclean[t] = 0u;
}

__global__ __launch_bounds__(256) void k_depth_view(const float *src, uint8_t *dst, uint32_t W, uint32_t H)
{
    const size_t n = (size_t)W * H;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t y = (uint32_t)(i / W), x = (uint32_t)(i % W);
        const uint8_t v = (uint8_t)f32_to_u8(src[i]);
        uint8_t *p = dst + ((size_t)(H - 1u - y) * W + x) * 3;
        p[0] = v;
        p[1] = v;
        p[2] = v;
    }
}

// Streaming a frame out to the host (app.rs:213-218 hands every frame to the window): one workgroup per tile of
// the scene's band writes the tile's rows straight into the page-locked HOST buffer -- or nothing at all: a tile
// whose colour-clean flag is up holds the cleared colour on the device, and if the host buffer's own flag says
// the tile was zeros the last time it was written there, nothing has to cross PCIe (three quarters of a
// 4096^2 frame of the reference's model).  `host_clean` belongs to (scene, host buffer); 16-byte pieces, so
// the launcher requires width % 16 == 0.
__global__ __launch_bounds__(256) void k_read_back(const uint8_t *__restrict__ fb, uint8_t *__restrict__ host,
                                                   const uint32_t *__restrict__ fb_clean, uint32_t *host_clean, DevFrame frame)
{
    const uint32_t t = blockIdx.x;
    const bool zeros = fb_clean[t] != 0u;
    const bool host_zeros = host_clean[t] != 0u;
    __syncthreads();  // (every thread has read the host flag before thread 0 changes it)
    if (zeros && host_zeros) return;
    const int32_t W = (int32_t)frame.width, H = (int32_t)frame.height;
    const int32_t x0 = (int32_t)(t % frame.ntx) * TILE_W, y0 = (frame.ty_base + (int32_t)(t / frame.ntx)) * TILE_H;
    // TILE_H rows x 24 pieces of 16 B
    for (uint32_t c = threadIdx.x; c < (uint32_t)TILE_H * 24u; c += 256u) {
        const int32_t y = y0 + (int32_t)(c / 24u);
        const int32_t xb = x0 * 3 + (int32_t)(c % 24u) * 16;
        if (xb < W * 3 && y >= frame.band_y0 && y < frame.band_y1) {
            const size_t at = (size_t)(H - 1 - y) * W * 3 + xb;
            const uint4 v = zeros ? make_uint4(0u, 0u, 0u, 0u) : *reinterpret_cast<const uint4 *>(fb + at);
            *reinterpret_cast<uint4 *>(host + at) = v;
        }
    }
    if (threadIdx.x == 0u) host_clean[t] = zeros ? 1u : 0u;
}

// The sparse form of the frame exchange between GPUs (tr_exchange_all_gather_tiles): this rank's band goes to a
// peer's copy of the frame tile by tile, like k_read_back to the host -- a tile whose colour-clean flag is up holds
// zeros here, and if this rank's record of the PEER's copy (`remote_clean`, kept by the exchange per slot and peer)
// says the tile was zeros the last time it was written there, nothing crosses the link: three quarters of a 4096^2
// frame of the reference's model.  `peer` is the peer's frame slot mapped into this process (HIP IPC); the stores
// are plain stores over xGMI, made visible by the kernel's end and the system-scope flag store that follows it on
// the stream.  `poisoned`: the exchange's error word -- after a peer failed to open its slot in time nothing is
// written into it.  `bytes`: running count of what was pushed.
__global__ __launch_bounds__(256) void k_push_tiles(const uint8_t *__restrict__ fb, uint8_t *__restrict__ peer,
                                                    const uint32_t *__restrict__ fb_clean, uint32_t *remote_clean, DevFrame frame,
                                                    const uint32_t *poisoned, unsigned long long *bytes)
{
    // one load of the error word per workgroup, then a uniform branch: a time-out raised on another copy stream
    // while this kernel runs must not split the workgroup around the barrier
    __shared__ uint32_t s_poisoned;
    if (threadIdx.x == 0u) s_poisoned = __hip_atomic_load(poisoned, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    const uint32_t t = blockIdx.x;
    const bool zeros = fb_clean[t] != 0u;
    const bool remote_zeros = remote_clean[t] != 0u;
    __syncthreads();  // (every thread has read the remote flag before thread 0 changes it)
    if (s_poisoned != 0u) return;
    if (zeros && remote_zeros) return;
    const int32_t W = (int32_t)frame.width, H = (int32_t)frame.height;
    const int32_t x0 = (int32_t)(t % frame.ntx) * TILE_W, y0 = (frame.ty_base + (int32_t)(t / frame.ntx)) * TILE_H;
    uint32_t pieces = 0;
    // TILE_H rows x 24 pieces of 16 B
    for (uint32_t c = threadIdx.x; c < (uint32_t)TILE_H * 24u; c += 256u) {
        const int32_t y = y0 + (int32_t)(c / 24u);
        const int32_t xb = x0 * 3 + (int32_t)(c % 24u) * 16;
        if (xb < W * 3 && y >= frame.band_y0 && y < frame.band_y1) {
            const size_t at = (size_t)(H - 1 - y) * W * 3 + xb;
            const uint4 v = zeros ? make_uint4(0u, 0u, 0u, 0u) : *reinterpret_cast<const uint4 *>(fb + at);
            *reinterpret_cast<uint4 *>(peer + at) = v;
            pieces++;
        }
    }
    if (pieces) atomicAdd(bytes, (unsigned long long)pieces * 16ull);
    if (threadIdx.x == 0u) remote_clean[t] = zeros ? 1u : 0u;
}

// Supersampled output (tr_scene_resolve): the band's frame, box-filtered by F = 2, 4 or 8 on its stored u8 values
// (tr_resolve.h) into a frame of width / F x height / F pixels.  Tiles are the 128 x 16 source tiles of k_read_back;
// F divides both sides and the launcher's caller requires width, height and the band's rows to be multiples of F, so
// a source block never straddles a tile or the band.  A tile whose colour-clean flag is up holds the cleared colour:
// it is not read, its output pixels are stored as zeros (three quarters of a frame of the reference's model).
// A lane takes 16 source pixels -- three 16-byte pieces -- of each of F rows and owns the 16 / F output pixels below
// them; lanes run along the row first.  A tile has 8 * 16 / F such shares, a wavefront takes 64 of them: one tile at
// F = 2, two at 4, four at 8.  WIDE: width % 16 == 0 and both buffers aligned for 16-byte loads and 8 / 4 / 2-byte
// stores (the launcher checks); otherwise the same shares through byte loads and stores, which also serves the
// last columns of a width that is not a multiple of 16.
template <int F, bool WIDE>
__global__ __launch_bounds__(64) void k_resolve(const uint8_t *__restrict__ fb, uint8_t *__restrict__ out,
                                                const uint32_t *__restrict__ fb_clean, DevFrame frame)
{
    constexpr uint32_t SHARES = 8u * (uint32_t)(TILE_H / F);  // of one tile: 64, 32, 16
    constexpr int OUT_BYTES = 48 / F, OUT_WORDS = (OUT_BYTES + 3) / 4;
    const uint32_t t = blockIdx.x * (64u / SHARES) + threadIdx.x / SHARES;
    if (t >= frame.ntx * frame.nty) return;
    const uint32_t share = threadIdx.x % SHARES;
    const int32_t W = (int32_t)frame.width, H = (int32_t)frame.height;
    const int32_t x = (int32_t)(t % frame.ntx) * TILE_W + (int32_t)(share % 8u) * 16;
    const int32_t y = (frame.ty_base + (int32_t)(t / frame.ntx)) * TILE_H + (int32_t)(share / 8u) * F;  // lowest of the F rows
    if (x >= W || y < frame.band_y0 || y + F > frame.band_y1) return;
    const bool zeros = fb_clean != nullptr && fb_clean[t] != 0u;
    const int32_t row = H - y - F;  // first of the F buffer rows (row 0 = top); output row = row / F
    const int32_t n_bytes = min(16, W - x) * 3;  // of a source row (WIDE: always 48)
    uint32_t res[OUT_WORDS];
    if (zeros) {
#pragma unroll
        for (int w = 0; w < OUT_WORDS; w++) res[w] = 0u;
    } else {
        uint32_t src[F * 12];
        const uint8_t *p = fb + ((size_t)row * (size_t)W + (size_t)x) * 3u;
#pragma unroll
        for (int r = 0; r < F; r++) {
            const uint8_t *q = p + (size_t)r * (size_t)W * 3u;
            if (WIDE) {
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const uint4 v = *reinterpret_cast<const uint4 *>(q + 16 * k);
                    src[r * 12 + 4 * k + 0] = v.x;
                    src[r * 12 + 4 * k + 1] = v.y;
                    src[r * 12 + 4 * k + 2] = v.z;
                    src[r * 12 + 4 * k + 3] = v.w;
                }
            } else {
#pragma unroll
                for (int w = 0; w < 12; w++) {
                    uint32_t v = 0u;
#pragma unroll
                    for (int b = 0; b < 4; b++)
                        if (4 * w + b < n_bytes) v |= (uint32_t)q[4 * w + b] << (8 * b);
                    src[r * 12 + w] = v;
                }
            }
        }
        resolve_block<F>(src, res);
    }
    uint8_t *o = out + ((size_t)(row / F) * (size_t)(W / F) + (size_t)(x / F)) * 3u;
    if (WIDE) {
        if (F == 2) {
#pragma unroll
            for (int k = 0; k < 3; k++) reinterpret_cast<uint2 *>(o)[k] = make_uint2(res[2 * k], res[2 * k + 1]);
        } else if (F == 4) {
#pragma unroll
            for (int k = 0; k < 3; k++) reinterpret_cast<uint32_t *>(o)[k] = res[k];
        } else {
#pragma unroll
            for (int k = 0; k < 3; k++) reinterpret_cast<uint16_t *>(o)[k] = (uint16_t)(res[k >> 1] >> (16 * (k & 1)));
        }
    } else {
#pragma unroll
        for (int b = 0; b < OUT_BYTES; b++)
            if (b * F < n_bytes) o[b] = (uint8_t)(res[b >> 2] >> (8 * (b & 3)));
    }
}

// Depth compositing (tr_scene_composite): scene src's current frame merged into scene dst's by the reference's depth
// test (tr_composite.h has the rule).  One workgroup per 128 x 16 tile of dst's band, the tiles of k_read_back and
// k_resolve; a lane owns 16 pixels of a row -- four 16-byte pieces of z, three of colour, four of winner words -- and
// lanes run along the row first.
//   * src's z flag up: nothing of src is drawn in the tile (its z memory means nothing) -- the workgroup leaves having
//     loaded one word, before any barrier (three quarters of a frame of the reference's model);
//   * dst's z flag up: every zd is f32::MIN, dst's z memory is not read;
//   * the only barrier is the workgroup's vote "did any pixel win" (it also separates every lane's load of dst's z
//     flag from lane 0's store to it).  No winner: dst's memory and flags are untouched;
//   * otherwise lanes with a winning pixel load src's and dst's colour pieces, merge the winning pixels' bytes into
//     what they read and store the pieces back, and store the merged z (and winner words); if dst's z flag was up
//     EVERY lane inside the band and the width stores its z -- the rest of the tile as f32::MIN, as
//     k_materialize_depth would -- and the flag comes down; dst's colour-clean flag comes down.
// dst's colour needs no such care: a colour-clean tile holds real zeros.  Bytes per pixel of a tile that is read:
// 4 + 4 + 3 + 3 read, up to 4 + 3 written (8 more each way with winner taps).
// WIDE: width % 16 == 0 and every buffer 16-byte aligned (the launcher checks); otherwise the same shares through
// element loads and stores guarded by the width, which also serve the last columns of a width that is not a
// multiple of 16.  No LDS beyond the vote, no atomics, no scratch.
template <bool WIDE>
__global__ __launch_bounds__(8 * TILE_H) void k_composite(CompositeArgs a)
{
    static_assert(TILE_W == 128, "a row of a tile is eight shares of 16 pixels");
    const uint32_t t = blockIdx.x;
    if (a.src_zclean[t] != 0u) return;  // (workgroup-uniform, ahead of the barrier)
    const bool dz_clean = a.dst_zclean[t] != 0u;
    const int32_t W = (int32_t)a.frame.width, H = (int32_t)a.frame.height;
    const int32_t x = (int32_t)(t % a.frame.ntx) * TILE_W + (int32_t)(threadIdx.x % 8u) * 16;
    const int32_t y = (a.frame.ty_base + (int32_t)(t / a.frame.ntx)) * TILE_H + (int32_t)(threadIdx.x / 8u);
    const bool inside = x < W && y >= a.frame.band_y0 && y < a.frame.band_y1;
    const int32_t n_px = inside ? min(16, W - x) : 0;  // pixels of the share (WIDE: 16 or none)
    const size_t zi = inside ? (size_t)y * (size_t)W + (size_t)x : 0u;
    float zd[16];
    uint32_t won = 0u;  // bit i: pixel i of the share takes src's fragment
    if (inside) {
        float zs[16];
        if (WIDE) {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const float4 s = reinterpret_cast<const float4 *>(a.src_z + zi)[k];
                zs[4 * k + 0] = s.x, zs[4 * k + 1] = s.y, zs[4 * k + 2] = s.z, zs[4 * k + 3] = s.w;
                float4 d = make_float4(bits_f32(TR_F32_MIN_BITS), bits_f32(TR_F32_MIN_BITS), bits_f32(TR_F32_MIN_BITS),
                                       bits_f32(TR_F32_MIN_BITS));
                if (!dz_clean) d = reinterpret_cast<const float4 *>(a.dst_z + zi)[k];
                zd[4 * k + 0] = d.x, zd[4 * k + 1] = d.y, zd[4 * k + 2] = d.z, zd[4 * k + 3] = d.w;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 16; i++) {
                zs[i] = zd[i] = bits_f32(TR_F32_MIN_BITS);
                if (i < n_px) {
                    zs[i] = a.src_z[zi + i];
                    if (!dz_clean) zd[i] = a.dst_z[zi + i];
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 16; i++)
            if (composite_wins(zs[i], zd[i])) {
                won |= 1u << i;
                zd[i] = zs[i];
            }
    }
    if (__syncthreads_or((int)won) == 0) return;  // nothing of the tile changes
    if (threadIdx.x == 0u) {
        a.dst_fbclean[t] = 0u;
        if (dz_clean) a.dst_zclean[t] = 0u;
    }
    if (!inside) return;
    if (won != 0u || dz_clean) {  // the merged z: the winners', and a materialised tile's every pixel
        if (WIDE) {
#pragma unroll
            for (int k = 0; k < 4; k++)
                reinterpret_cast<float4 *>(a.dst_z + zi)[k] = make_float4(zd[4 * k], zd[4 * k + 1], zd[4 * k + 2], zd[4 * k + 3]);
        } else {
#pragma unroll
            for (int i = 0; i < 16; i++)
                if (i < n_px && (dz_clean || ((won >> i) & 1u))) a.dst_z[zi + i] = zd[i];
        }
    }
    if (won == 0u) return;
    const size_t ci = ((size_t)(H - 1 - y) * (size_t)W + (size_t)x) * 3u;
    if (WIDE) {
        uint32_t s[12], d[12];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const uint4 u = reinterpret_cast<const uint4 *>(a.src_fb + ci)[k];
            const uint4 v = reinterpret_cast<const uint4 *>(a.dst_fb + ci)[k];
            s[4 * k + 0] = u.x, s[4 * k + 1] = u.y, s[4 * k + 2] = u.z, s[4 * k + 3] = u.w;
            d[4 * k + 0] = v.x, d[4 * k + 1] = v.y, d[4 * k + 2] = v.z, d[4 * k + 3] = v.w;
        }
        // byte b of the share belongs to pixel b / 3: a mask per word from the pixels' bits
#pragma unroll
        for (int w = 0; w < 12; w++) {
            uint32_t m = 0u;
#pragma unroll
            for (int b = 0; b < 4; b++)
                if ((won >> ((4 * w + b) / 3)) & 1u) m |= 0xFFu << (8 * b);
            d[w] = (d[w] & ~m) | (s[w] & m);
        }
#pragma unroll
        for (int k = 0; k < 3; k++)
            reinterpret_cast<uint4 *>(a.dst_fb + ci)[k] = make_uint4(d[4 * k], d[4 * k + 1], d[4 * k + 2], d[4 * k + 3]);
    } else {
#pragma unroll
        for (int i = 0; i < 16; i++)
            if (i < n_px && ((won >> i) & 1u)) {
#pragma unroll
                for (int c = 0; c < 3; c++) a.dst_fb[ci + 3 * i + c] = a.src_fb[ci + 3 * i + c];
            }
    }
    if (a.dst_winner != nullptr) {
        if (WIDE) {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (((won >> (4 * k)) & 0xFu) == 0u) continue;
                const uint4 u = reinterpret_cast<const uint4 *>(a.src_winner + zi)[k];
                uint4 v = reinterpret_cast<const uint4 *>(a.dst_winner + zi)[k];
                if ((won >> (4 * k + 0)) & 1u) v.x = composite_winner(u.x, a.winner_base);
                if ((won >> (4 * k + 1)) & 1u) v.y = composite_winner(u.y, a.winner_base);
                if ((won >> (4 * k + 2)) & 1u) v.z = composite_winner(u.z, a.winner_base);
                if ((won >> (4 * k + 3)) & 1u) v.w = composite_winner(u.w, a.winner_base);
                reinterpret_cast<uint4 *>(a.dst_winner + zi)[k] = v;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 16; i++)
                if (i < n_px && ((won >> i) & 1u)) a.dst_winner[zi + i] = composite_winner(a.src_winner[zi + i], a.winner_base);
        }
    }
}

// Shared shadows (tr_scene_shadow_merge): scene src's shadow buffer merged into scene dst's by the reference's
// light-space test (tr_shadow_merge.h has the rule).  One workgroup of 256 lanes per 128 x 16 tile of the WHOLE frame
// (a shadow buffer is full-frame on a band scene too); a tile is 16 rows of 32 four-pixel pieces, a lane owns the piece
// at column 4 * (lane % 32) of rows lane / 32 and lane / 32 + 8, lanes run along the row first: a wavefront's load is
// two contiguous 512-byte row segments.  Decided on the two fast-clear flags:
//   * src's flag up: every value of src's tile is f32::MIN, which replaces nothing -- the workgroup leaves having loaded
//     one word, before any barrier;
//   * src's down, dst's up: every zd is f32::MIN and dst's stale memory is not read; every pixel of the tile inside the
//     frame is stored and the flag comes down.  The one barrier separates every lane's load of dst's flag from lane 0's
//     store to it (the branch is workgroup-uniform: all lanes read the same word);
//   * both down: elementwise; a piece is stored only where the merge changed a bit of it.
// The stores and the lowered flag are ordered before the colour pass that follows on the stream by the kernel boundary.
// WIDE: width % 4 == 0 and both buffers 16-byte aligned (the launcher checks): a piece is one 16-byte load per buffer
// and one store, and lies wholly inside or outside the row; otherwise the same pieces through element loads and stores
// guarded by the width.  Bytes per pixel of a tile that is read: 4 + 4 read, up to 4 written.  No LDS, no atomics.
template <bool WIDE>
__global__ __launch_bounds__(256) void k_shadow_merge(ShadowMergeArgs a)
{
    static_assert(TILE_W == 128 && TILE_H == 16, "a tile is 16 rows of 32 four-pixel pieces, two pieces per lane");
    const uint32_t t = blockIdx.x;
    if (a.src_clean[t] != 0u) return;  // (workgroup-uniform, ahead of the barrier)
    const bool d_clean = a.dst_clean[t] != 0u;
    if (d_clean) {
        __syncthreads();
        if (threadIdx.x == 0u) a.dst_clean[t] = 0u;
    }
    const int32_t W = (int32_t)a.frame.width;
    const int32_t x = (int32_t)(t % a.frame.ntx) * TILE_W + (int32_t)(threadIdx.x % 32u) * 4;
    const int32_t y0 = (a.frame.ty_base + (int32_t)(t / a.frame.ntx)) * TILE_H + (int32_t)(threadIdx.x / 32u);
    const float fmin = bits_f32(TR_F32_MIN_BITS);
    float zs[2][4], zd[2][4];
    size_t at[2];
    int32_t n_px[2];  // pixels of the piece inside the frame (WIDE: 4 or none)
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const int32_t y = y0 + 8 * r;
        const bool inside = x < W && y >= a.frame.band_y0 && y < a.frame.band_y1;
        n_px[r] = inside ? min(4, W - x) : 0;
        at[r] = inside ? (size_t)y * (size_t)W + (size_t)x : 0u;
#pragma unroll
        for (int i = 0; i < 4; i++) zs[r][i] = zd[r][i] = fmin;
        if (n_px[r] == 0) continue;
        if (WIDE) {
            const float4 s = *reinterpret_cast<const float4 *>(a.src + at[r]);
            zs[r][0] = s.x, zs[r][1] = s.y, zs[r][2] = s.z, zs[r][3] = s.w;
            if (!d_clean) {
                const float4 d = *reinterpret_cast<const float4 *>(a.dst + at[r]);
                zd[r][0] = d.x, zd[r][1] = d.y, zd[r][2] = d.z, zd[r][3] = d.w;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++)
                if (i < n_px[r]) {
                    zs[r][i] = a.src[at[r] + i];
                    if (!d_clean) zd[r][i] = a.dst[at[r] + i];
                }
        }
    }
#pragma unroll
    for (int r = 0; r < 2; r++) {
        if (n_px[r] == 0) continue;
        float m[4];
        uint32_t changed = 0u;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            m[i] = shadow_merge(zs[r][i], zd[r][i]);
            if (f32_bits(m[i]) != f32_bits(zd[r][i])) changed |= 1u << i;
        }
        if (WIDE) {
            if (d_clean || changed != 0u) *reinterpret_cast<float4 *>(a.dst + at[r]) = make_float4(m[0], m[1], m[2], m[3]);
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++)
                if (i < n_px[r] && (d_clean || ((changed >> i) & 1u))) a.dst[at[r] + i] = m[i];
        }
    }
}

// Screen-space ambient occlusion (tr_scene_ambient_occlusion): the frame's colour darkened in place from its own z
// buffer (tr_ao.h has the rule).  One workgroup of 256 lanes per 128 x 16 tile of the frame, the tiles of k_composite.
//   * the tile's own z flag up: nothing is drawn there -- the workgroup leaves having loaded one word, before any barrier;
//   * staging: the tile's z and a halo of `radius` pixels go to LDS, as rows of 160 floats that start 16 pixels left of
//     the tile, so that every 16-byte piece of a row is aligned in memory and lies in ONE tile: a piece in a tile whose z
//     flag is up (its z memory is stale), or outside the frame, is filled with f32::MIN without a load.  The nine flags
//     are workgroup-uniform: scalar loads, one bit each.  At most 48 rows: 30 KB;
//   * samples: a lane owns one column of the tile and eight of its rows; lanes run along the row, so the 64 reads of a
//     sample hit 64 consecutive words of LDS.  The offset of a sample is uniform (the table is a kernel argument), the
//     eight rows are immediate offsets from it.  A pixel's samples are taken in the rule's order;
//   * the coefficients go through 8 KB of LDS to the colour shares of k_composite -- a lane owns 16 pixels of a row,
//     three 16-byte pieces -- behind the only other barrier, which is also the vote "is any pixel of the tile drawn";
//     no: the workgroup leaves.  A lane loads, blends and stores its pieces only if a pixel of its share changes (a
//     drawn pixel whose coefficient is 1 keeps its bytes: 1 * c + 0 * 0 = c);
//   * TR_AO_GREY: drawn pixels become coef * 255 whatever they held, so the tile's colour-clean flag comes down (lane 0,
//     behind the barrier).  Without it zeros blend to zeros and no flag changes.
// z and the flags of z are only read.  WIDE: width % 16 == 0 and both buffers 16-byte aligned (the launcher checks);
// otherwise the same through element accesses guarded by the width.  No atomics, no scratch.
constexpr int AO_LDS_W = TILE_W + 2 * AO_MAX_RADIUS, AO_LDS_H = TILE_H + 2 * AO_MAX_RADIUS;
constexpr int AO_THREADS = 256, AO_ROWS = TILE_W * TILE_H / AO_THREADS;  // rows of its column a lane owns
constexpr float AO_NOT_DRAWN = 2.0f;  // (in place of a coefficient, which never exceeds 1)
template <bool WIDE>
__global__ __launch_bounds__(AO_THREADS) void k_ao(AoArgs a)
{
    static_assert(TILE_W == 128 && AO_MAX_RADIUS == 16 && AO_MAX_RADIUS <= TILE_H, "the halo lies in the eight tiles around");
    const uint32_t t = blockIdx.x;
    if (a.zclean[t] != 0u) return;  // (workgroup-uniform, ahead of the barriers)
    __shared__ float s_z[AO_LDS_H * AO_LDS_W];
    __shared__ float s_coef[TILE_H * TILE_W];
    const int32_t W = (int32_t)a.frame.width, H = (int32_t)a.frame.height, R = (int32_t)a.radius;
    const int32_t ntx = (int32_t)a.frame.ntx, nty = (int32_t)a.frame.nty;
    const int32_t tx = (int32_t)t % ntx, ty = (int32_t)t / ntx;
    const int32_t x0 = tx * TILE_W, y0 = ty * TILE_H;
    // bit 3 * ay + ax: the tile at (tx + ax - 1, ty + ay - 1) reads as f32::MIN -- flag up, or no such tile
    uint32_t stale = 0u;
#pragma unroll
    for (int32_t ay = 0; ay < 3; ay++)
#pragma unroll
        for (int32_t ax = 0; ax < 3; ax++) {
            const int32_t nx = tx + ax - 1, ny = ty + ay - 1;
            bool up = nx < 0 || nx >= ntx || ny < 0 || ny >= nty;
            if (!up) up = a.zclean[ny * ntx + nx] != 0u;
            if (up) stale |= 1u << (3 * ay + ax);
        }
    const int32_t rows = TILE_H + 2 * R;  // LDS row r is frame row y0 - R + r, LDS column c frame column x0 - 16 + c
    const float z_min = bits_f32(TR_F32_MIN_BITS);
    if (WIDE) {
        for (int32_t p = (int32_t)threadIdx.x; p < rows * (AO_LDS_W / 4); p += AO_THREADS) {
            const int32_t r = p / (AO_LDS_W / 4), j = p % (AO_LDS_W / 4);
            if (4 * j + 3 < 16 - R || 4 * j >= 16 + TILE_W + R) continue;  // (no sample reaches it)
            const int32_t x = x0 - 16 + 4 * j, y = y0 - R + r;
            const int32_t ax = j < 4 ? 0 : j < 4 + TILE_W / 4 ? 1 : 2, ay = y < y0 ? 0 : y < y0 + TILE_H ? 1 : 2;
            float4 v = make_float4(z_min, z_min, z_min, z_min);
            if (((stale >> (3 * ay + ax)) & 1u) == 0u && x < W && y < H)
                v = *reinterpret_cast<const float4 *>(a.z + (size_t)y * (size_t)W + (size_t)x);
            *reinterpret_cast<float4 *>(&s_z[r * AO_LDS_W + 4 * j]) = v;
        }
    } else {
        for (int32_t p = (int32_t)threadIdx.x; p < rows * AO_LDS_W; p += AO_THREADS) {
            const int32_t r = p / AO_LDS_W, c = p % AO_LDS_W;
            if (c < 16 - R || c >= 16 + TILE_W + R) continue;
            const int32_t x = x0 - 16 + c, y = y0 - R + r;
            const int32_t ax = c < 16 ? 0 : c < 16 + TILE_W ? 1 : 2, ay = y < y0 ? 0 : y < y0 + TILE_H ? 1 : 2;
            float v = z_min;
            if (((stale >> (3 * ay + ax)) & 1u) == 0u && x < W && y < H) v = a.z[(size_t)y * (size_t)W + (size_t)x];
            s_z[r * AO_LDS_W + c] = v;
        }
    }
    __syncthreads();
    // samples: column `col`, rows row0 .. row0 + AO_ROWS - 1 of the tile
    const int32_t col = (int32_t)threadIdx.x % TILE_W, row0 = (int32_t)threadIdx.x / TILE_W * AO_ROWS;
    const float *own = s_z + (R + row0) * AO_LDS_W + 16 + col;
    float z0[AO_ROWS], coef[AO_ROWS];
    uint32_t drawn = 0u;
#pragma unroll
    for (int k = 0; k < AO_ROWS; k++) {
        z0[k] = own[k * AO_LDS_W];
        coef[k] = 1.0f;
        if (ao_drawn(z0[k])) drawn |= 1u << k;
    }
    if (drawn != 0u)
        for (uint32_t i = 0; i < a.n_taps; i++) {
            const int32_t off = (int32_t)a.taps.d[i][1] * AO_LDS_W + (int32_t)a.taps.d[i][0];
#pragma unroll
            for (int k = 0; k < AO_ROWS; k++)
                if ((drawn >> k) & 1u) coef[k] = ao_sample(coef[k], z0[k], own[off + k * AO_LDS_W], a.rule);
        }
#pragma unroll
    for (int k = 0; k < AO_ROWS; k++) s_coef[(row0 + k) * TILE_W + col] = ((drawn >> k) & 1u) ? coef[k] : AO_NOT_DRAWN;
    if (__syncthreads_or((int)drawn) == 0) return;  // nothing of the tile is drawn
    const bool grey = a.grey != 0u;
    if (grey && threadIdx.x == 0u) a.fbclean[t] = 0u;
    // colour: the shares of k_composite
    if (threadIdx.x >= 8u * TILE_H) return;
    const int32_t x = x0 + (int32_t)(threadIdx.x % 8u) * 16, row = (int32_t)(threadIdx.x / 8u), y = y0 + row;
    if (x >= W || y >= H) return;
    const int32_t n_px = min(16, W - x);  // (WIDE: 16)
    float cf[16];
    uint32_t is_drawn = 0u, changes = 0u;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const float4 v = *reinterpret_cast<const float4 *>(&s_coef[row * TILE_W + (x - x0) + 4 * k]);
        cf[4 * k + 0] = v.x, cf[4 * k + 1] = v.y, cf[4 * k + 2] = v.z, cf[4 * k + 3] = v.w;
    }
#pragma unroll
    for (int i = 0; i < 16; i++) {
        if (cf[i] != AO_NOT_DRAWN) {
            is_drawn |= 1u << i;
            if (grey || cf[i] != 1.0f) changes |= 1u << i;
        } else {
            cf[i] = 1.0f;  // (keeps every byte)
        }
    }
    if (changes == 0u) return;
    const size_t ci = ((size_t)(H - 1 - y) * (size_t)W + (size_t)x) * 3u;
    if (WIDE) {
        uint32_t w[12];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const uint4 u = reinterpret_cast<const uint4 *>(a.fb + ci)[k];
            w[4 * k + 0] = u.x, w[4 * k + 1] = u.y, w[4 * k + 2] = u.z, w[4 * k + 3] = u.w;
        }
        // byte b of the share is channel b % 3 of pixel b / 3
#pragma unroll
        for (int b = 0; b < 48; b++) {
            const int i = b / 3, sh = 8 * (b % 4);
            const uint32_t c = (grey && ((is_drawn >> i) & 1u)) ? 255u : (w[b / 4] >> sh) & 0xFFu;
            w[b / 4] = (w[b / 4] & ~(0xFFu << sh)) | (ao_channel(c, cf[i]) << sh);
        }
#pragma unroll
        for (int k = 0; k < 3; k++)
            reinterpret_cast<uint4 *>(a.fb + ci)[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
    } else {
#pragma unroll
        for (int i = 0; i < 16; i++)
            if (i < n_px && ((changes >> i) & 1u)) {
#pragma unroll
                for (int ch = 0; ch < 3; ch++) {
                    const uint32_t c = grey ? 255u : (uint32_t)a.fb[ci + 3 * i + ch];
                    a.fb[ci + 3 * i + ch] = (uint8_t)ao_channel(c, cf[i]);
                }
            }
    }
}

// Frame accumulation (tr_scene_accumulate): n kept frames of a call averaged under integer weights into `out`, byte by
// byte on their stored u8 values (tr_accumulate.h has the rule).  One workgroup per 128 x 16 tile of the band, the tiles
// of k_read_back and k_composite; a lane owns 16 pixels of a row -- three 16-byte pieces -- and lanes run along the row
// first.  Frame pointers, flag pointers, weights and the divisor's constants are kernel arguments.
//   * per tile the n colour-clean flags are workgroup-uniform (scalar loads); a frame whose flag is up holds zeros
//     there and one of weight 0 counts for nothing: neither is read.  The others are the tile's contributors;
//   * no contributor: every byte of the tile is (0 + D / 2) / D = 0.  Out of place the zeros are stored without a load;
//     in place (out is one of the frames, out_clean its flags) a destination whose own flag is up holds them already and
//     the workgroup leaves -- a destination that is drawn there but weighs nothing is zeroed;
//   * otherwise a lane loads its pieces of every contributor, multiplies and adds byte by byte in 32-bit accumulators that
//     start at D / 2, divides by the multiplier and shift of accumulate_div and stores its three pieces.  It has read
//     its pieces of every frame before it writes them, and no other lane touches them: in place is safe;
//   * in place over a destination flag that is up the tile now holds the average of what the others drew: lane 0 lowers
//     the flag behind a barrier (every wave has read the flags by then), or k_resolve and the sparse read-back would
//     take the tile for zeros.
// WIDE: width % 16 == 0 and every buffer 16-byte aligned (the launcher checks); otherwise the same shares through byte
// accesses guarded by the width, which also serve the last columns of a width that is not a multiple of 16.  Rows
// outside the band are not touched.  No atomics, no LDS beyond the barrier, no scratch.
template <bool WIDE>
__global__ __launch_bounds__(8 * TILE_H) void k_accumulate(AccumulateArgs a)
{
    static_assert(TILE_W == 128, "a row of a tile is eight shares of 16 pixels");
    const uint32_t t = blockIdx.x;
    uint32_t contrib = 0u;  // bit k: frame k is read
    for (uint32_t k = 0; k < a.n; k++) {
        const uint32_t *flags = a.clean[k];
        const bool zeros = a.w[k] == 0u || (flags != nullptr && flags[t] != 0u);
        if (!zeros) contrib |= 1u << k;
    }
    const bool out_was_clean = a.out_clean != nullptr && a.out_clean[t] != 0u;
    if (contrib == 0u && out_was_clean) return;  // (workgroup-uniform, ahead of the barrier)
    const int32_t W = (int32_t)a.frame.width, H = (int32_t)a.frame.height;
    const int32_t x = (int32_t)(t % a.frame.ntx) * TILE_W + (int32_t)(threadIdx.x % 8u) * 16;
    const int32_t y = (a.frame.ty_base + (int32_t)(t / a.frame.ntx)) * TILE_H + (int32_t)(threadIdx.x / 8u);
    const bool inside = x < W && y >= a.frame.band_y0 && y < a.frame.band_y1;
    if (inside) {
        const int32_t n_bytes = min(16, W - x) * 3;  // of the share (WIDE: 48)
        const size_t ci = ((size_t)(H - 1 - y) * (size_t)W + (size_t)x) * 3u;
        uint32_t res[12];
        if (contrib == 0u) {
#pragma unroll
            for (int w = 0; w < 12; w++) res[w] = 0u;
        } else {
            uint32_t acc[48];
#pragma unroll
            for (int b = 0; b < 48; b++) acc[b] = a.div.half;
            for (uint32_t k = 0; k < a.n; k++) {
                if (((contrib >> k) & 1u) == 0u) continue;
                const uint8_t *p = a.fb[k] + ci;
                const uint32_t wk = a.w[k] & 0xFFu;  // (<= 255, the launcher checks: a 24-bit multiply-add per byte)
                uint32_t v[12];
                if (WIDE) {
#pragma unroll
                    for (int q = 0; q < 3; q++) {
                        const uint4 u = reinterpret_cast<const uint4 *>(p)[q];
                        v[4 * q + 0] = u.x, v[4 * q + 1] = u.y, v[4 * q + 2] = u.z, v[4 * q + 3] = u.w;
                    }
                } else {
#pragma unroll
                    for (int w = 0; w < 12; w++) {
                        uint32_t u = 0u;
#pragma unroll
                        for (int b = 0; b < 4; b++)
                            if (4 * w + b < n_bytes) u |= (uint32_t)p[4 * w + b] << (8 * b);
                        v[w] = u;
                    }
                }
#pragma unroll
                for (int b = 0; b < 48; b++) acc[b] += wk * ((v[b >> 2] >> (8 * (b & 3))) & 0xFFu);
            }
#pragma unroll
            for (int w = 0; w < 12; w++) {
                res[w] = 0u;
#pragma unroll
                for (int b = 0; b < 4; b++) res[w] |= accumulate_div(acc[4 * w + b], a.div) << (8 * b);
            }
        }
        uint8_t *o = a.out + ci;
        if (WIDE) {
#pragma unroll
            for (int q = 0; q < 3; q++)
                reinterpret_cast<uint4 *>(o)[q] = make_uint4(res[4 * q], res[4 * q + 1], res[4 * q + 2], res[4 * q + 3]);
        } else {
#pragma unroll
            for (int b = 0; b < 48; b++)
                if (b < n_bytes) o[b] = (uint8_t)(res[b >> 2] >> (8 * (b & 3)));
        }
    }
    if (!out_was_clean || contrib == 0u) return;  // (workgroup-uniform)
    __syncthreads();
    if (threadIdx.x == 0u) a.out_clean[t] = 0u;
}

// Depth of field (tr_scene_depth_of_field): the frame's colour blurred by its own z buffer into `out`, never in place
// (a tap reads a neighbour's colour); tr_dof.h has the rule.  One workgroup of 256 lanes per 128 x 16 tile of the frame,
// the tiles of k_ao.  The nine z flags and nine colour flags of the 3 x 3 neighbourhood are workgroup-uniform.
//   * TR_DOF_SHOW_COC: a lane of the colour shares loads its 16 depths (none if the tile's z flag is up) and stores the
//     grey circles; no LDS, no barrier;
//   * all nine colour flags up (a tile outside the grid counts as up): every tap is black, the tile is zeros whatever
//     the circles are -- stored without loading a pixel, ahead of any barrier;
//   * staging: the tile and a halo of max_radius pixels go to LDS as rows of 160 pairs {packed pixel, wt[coc]} that
//     start 16 pixels left of the tile, so that a 16-byte piece of z is aligned in memory and lies in ONE tile: a piece
//     in a tile whose z flag is up gets f32::MIN without a load, one in a tile whose colour flag is up zeros without a
//     load, and one outside the frame {0, wt[0]}: circle 0, which no tap at a distance >= 1 satisfies (only a lane whose
//     own pixel is outside the frame sees it, and its result is never stored).  16 + 2 R rows of 1280 bytes: 23 KB at
//     radius 1, 40 KB at radius 8 (dynamic LDS, so four to seven workgroups share a CU);
//   * the vote: the largest circle among the staged pixels, through a wave reduction and four words of LDS behind the
//     staging barrier.  No tap at a distance beyond it qualifies anywhere in the tile, so the loops run to it instead
//     of max_radius; zero: the tile is a plain copy of its colour;
//   * the gather: a lane owns one column of the tile and eight of its rows; lanes run along the row, so a tap reads 64
//     consecutive pairs (one ds_read_b64, no bank conflict).  dx and dy are loop variables: the distance is scalar, the
//     test one unsigned compare of the packed word, the weight a select, the sums four u32 per pixel (dof_tap);
//   * the results go through the first 8 KB of the same LDS (a barrier on either side) to the colour shares of
//     k_composite -- a lane owns 16 pixels of a row, three 16-byte pieces -- and every byte of the tile is stored;
//   * out_clean, when given, gets the tile's flag: 1 where the tile was stored as zeros on the flags alone (its own
//     colour flag was up, so its winner words are the cleared value too), 0 otherwise.
// z, fb and every flag of the frame are only read.  WIDE: width % 16 == 0 and z, fb and out 16-byte aligned (the launcher
// checks); otherwise the same through element accesses guarded by the width.  No atomics, no scratch.
constexpr int DOF_LDS_W = TILE_W + 32;
constexpr int DOF_THREADS = 256, DOF_ROWS = TILE_W * TILE_H / DOF_THREADS;  // rows of its column a lane owns

// The 16 finished pixels of a share (24 bits each) into `o`: three 16-byte pieces, or n_px * 3 guarded bytes.
template <bool WIDE>
__device__ __forceinline__ void dof_store_share(uint8_t *o, const uint32_t (&px)[16], int32_t n_px)
{
    if (WIDE) {
        uint32_t w[12];
#pragma unroll
        for (int g = 0; g < 4; g++) {
            w[3 * g + 0] = px[4 * g] | (px[4 * g + 1] << 24);
            w[3 * g + 1] = (px[4 * g + 1] >> 8) | (px[4 * g + 2] << 16);
            w[3 * g + 2] = (px[4 * g + 2] >> 16) | (px[4 * g + 3] << 8);
        }
#pragma unroll
        for (int k = 0; k < 3; k++) reinterpret_cast<uint4 *>(o)[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
    } else {
#pragma unroll
        for (int i = 0; i < 16; i++)
            if (i < n_px) {
                o[3 * i + 0] = (uint8_t)(px[i] & 0xFFu);
                o[3 * i + 1] = (uint8_t)((px[i] >> 8) & 0xFFu);
                o[3 * i + 2] = (uint8_t)((px[i] >> 16) & 0xFFu);
            }
    }
}

template <bool WIDE>
__global__ __launch_bounds__(DOF_THREADS) void k_dof(DofArgs a)
{
    static_assert(TILE_W == 128 && DOF_MAX_RADIUS <= 16 && DOF_MAX_RADIUS <= TILE_H, "the halo lies in the eight tiles around");
    static_assert(DOF_THREADS == 4 * 64 && 8 * TILE_H <= DOF_THREADS, "four waves vote; the shares are the first lanes");
    extern __shared__ uint2 s_px[];  // (TILE_H + 2 R) rows of DOF_LDS_W pairs; later the tile's results, one word each
    __shared__ uint32_t s_max[4];
    const uint32_t t = blockIdx.x;
    const int32_t W = (int32_t)a.frame.width, H = (int32_t)a.frame.height, R = (int32_t)a.rule.max_radius;
    const int32_t ntx = (int32_t)a.frame.ntx, nty = (int32_t)a.frame.nty;
    const int32_t tx = (int32_t)t % ntx, ty = (int32_t)t / ntx;
    const int32_t x0 = tx * TILE_W, y0 = ty * TILE_H;
    // bit 3 * ay + ax, the tile at (tx + ax - 1, ty + ay - 1): no such tile / its z reads as f32::MIN / its colour as zeros
    uint32_t none = 0u, zstale = 0u, czero = 0u;
#pragma unroll
    for (int32_t ay = 0; ay < 3; ay++)
#pragma unroll
        for (int32_t ax = 0; ax < 3; ax++) {
            const int32_t nx = tx + ax - 1, ny = ty + ay - 1;
            const uint32_t bit = 1u << (3 * ay + ax);
            if (nx < 0 || nx >= ntx || ny < 0 || ny >= nty) {
                none |= bit, zstale |= bit, czero |= bit;
            } else {
                if (a.zclean[ny * ntx + nx] != 0u) zstale |= bit;
                if (a.fbclean != nullptr && a.fbclean[ny * ntx + nx] != 0u) czero |= bit;
            }
        }
    const uint32_t own_bit = 1u << 4;
    // the colour shares of k_composite
    const int32_t sx = x0 + (int32_t)(threadIdx.x % 8u) * 16, srow = (int32_t)(threadIdx.x / 8u), sy = y0 + srow;
    const bool share = threadIdx.x < 8u * TILE_H && sx < W && sy < H;
    const int32_t n_px = share ? min(16, W - sx) : 0;  // (WIDE: 16 or none)
    uint8_t *o = share ? a.out + ((size_t)(H - 1 - sy) * (size_t)W + (size_t)sx) * 3u : nullptr;
    uint32_t px[16];
    if (a.show_coc != 0u) {  // (workgroup-uniform)
        if (a.out_clean != nullptr && threadIdx.x == 0u)
            a.out_clean[t] = ((czero & zstale & own_bit) != 0u && a.rule.background_radius == 0u) ? 1u : 0u;
        if (!share) return;
        const float *zp = a.z + (size_t)sy * (size_t)W + (size_t)sx;
        float zv[16];
#pragma unroll
        for (int i = 0; i < 16; i++) zv[i] = bits_f32(TR_F32_MIN_BITS);
        if ((zstale & own_bit) == 0u) {
            if (WIDE) {
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const float4 v = reinterpret_cast<const float4 *>(zp)[k];
                    zv[4 * k + 0] = v.x, zv[4 * k + 1] = v.y, zv[4 * k + 2] = v.z, zv[4 * k + 3] = v.w;
                }
            } else {
#pragma unroll
                for (int i = 0; i < 16; i++)
                    if (i < n_px) zv[i] = zp[i];
            }
        }
#pragma unroll
        for (int i = 0; i < 16; i++) px[i] = dof_show(dof_coc(zv[i], a.rule), a.rule.max_radius) * 0x010101u;
        dof_store_share<WIDE>(o, px, n_px);
        return;
    }
    const bool all_zero = czero == 0x1FFu;
    if (a.out_clean != nullptr && threadIdx.x == 0u) a.out_clean[t] = all_zero ? 1u : 0u;
    if (all_zero) {  // (workgroup-uniform, ahead of the barriers)
        if (!share) return;
#pragma unroll
        for (int i = 0; i < 16; i++) px[i] = 0u;
        dof_store_share<WIDE>(o, px, n_px);
        return;
    }
    const int32_t rows = TILE_H + 2 * R;  // LDS row r is frame row y0 - R + r, LDS column c frame column x0 - 16 + c
    uint32_t widest = 0u;                 // the largest circle this lane staged
    if (WIDE) {
        for (int32_t p = (int32_t)threadIdx.x; p < rows * (DOF_LDS_W / 4); p += DOF_THREADS) {
            const int32_t r = p / (DOF_LDS_W / 4), j = p % (DOF_LDS_W / 4);
            if (4 * j + 3 < 16 - R || 4 * j >= 16 + TILE_W + R) continue;  // (no tap reaches it)
            const int32_t x = x0 - 16 + 4 * j, y = y0 - R + r;
            const int32_t ax = j < 4 ? 0 : j < 4 + TILE_W / 4 ? 1 : 2, ay = y < y0 ? 0 : y < y0 + TILE_H ? 1 : 2;
            const uint32_t bit = 1u << (3 * ay + ax);
            const bool inside = (none & bit) == 0u && x < W && y < H;
            const float z_min = bits_f32(TR_F32_MIN_BITS);
            float zv[4] = { z_min, z_min, z_min, z_min };
            uint32_t c[4] = { 0u, 0u, 0u, 0u };
            if (inside && (zstale & bit) == 0u) {
                const float4 v = *reinterpret_cast<const float4 *>(a.z + (size_t)y * (size_t)W + (size_t)x);
                zv[0] = v.x, zv[1] = v.y, zv[2] = v.z, zv[3] = v.w;
            }
            if (inside && (czero & bit) == 0u) {
                // four pixels are twelve bytes at a multiple of four: three aligned words
                const uint32_t *q = reinterpret_cast<const uint32_t *>(a.fb + ((size_t)(H - 1 - y) * (size_t)W + (size_t)x) * 3u);
                const uint32_t w0 = q[0], w1 = q[1], w2 = q[2];
                c[0] = w0 & 0xFFFFFFu;
                c[1] = (w0 >> 24) | ((w1 & 0xFFFFu) << 8);
                c[2] = (w1 >> 16) | ((w2 & 0xFFu) << 16);
                c[3] = w2 >> 8;
            }
            uint32_t e[8];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t coc = inside ? dof_coc(zv[k], a.rule) : 0u;
                widest = max(widest, coc);
                e[2 * k] = c[k] | (coc << 24);
                e[2 * k + 1] = dof_weight(coc);
            }
            uint4 *d = reinterpret_cast<uint4 *>(&s_px[r * DOF_LDS_W + 4 * j]);
            d[0] = make_uint4(e[0], e[1], e[2], e[3]);
            d[1] = make_uint4(e[4], e[5], e[6], e[7]);
        }
    } else {
        for (int32_t p = (int32_t)threadIdx.x; p < rows * DOF_LDS_W; p += DOF_THREADS) {
            const int32_t r = p / DOF_LDS_W, c = p % DOF_LDS_W;
            if (c < 16 - R || c >= 16 + TILE_W + R) continue;
            const int32_t x = x0 - 16 + c, y = y0 - R + r;
            const int32_t ax = c < 16 ? 0 : c < 16 + TILE_W ? 1 : 2, ay = y < y0 ? 0 : y < y0 + TILE_H ? 1 : 2;
            const uint32_t bit = 1u << (3 * ay + ax);
            const bool inside = (none & bit) == 0u && x < W && y < H;
            float zv = bits_f32(TR_F32_MIN_BITS);
            uint32_t col = 0u;
            if (inside && (zstale & bit) == 0u) zv = a.z[(size_t)y * (size_t)W + (size_t)x];
            if (inside && (czero & bit) == 0u) {
                const uint8_t *q = a.fb + ((size_t)(H - 1 - y) * (size_t)W + (size_t)x) * 3u;
                col = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16);
            }
            const uint32_t coc = inside ? dof_coc(zv, a.rule) : 0u;
            widest = max(widest, coc);
            s_px[r * DOF_LDS_W + c] = make_uint2(col | (coc << 24), dof_weight(coc));
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) widest = max(widest, (uint32_t)__shfl_xor((int)widest, off));
    if (threadIdx.x % 64u == 0u) s_max[threadIdx.x / 64u] = widest;
    __syncthreads();
    const int32_t reach = (int32_t)__builtin_amdgcn_readfirstlane(max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3])));
    // the gather: column `col`, rows row0 .. row0 + DOF_ROWS - 1 of the tile
    const int32_t col = (int32_t)threadIdx.x % TILE_W, row0 = (int32_t)threadIdx.x / TILE_W * DOF_ROWS;
    const uint2 *own = s_px + (R + row0) * DOF_LDS_W + 16 + col;
    uint32_t res[DOF_ROWS];
    if (reach == 0) {  // (workgroup-uniform) every circle is 0: only q = p qualifies, (32768 c + 16384) / 32768 = c
#pragma unroll
        for (int k = 0; k < DOF_ROWS; k++) res[k] = own[k * DOF_LDS_W].x & 0xFFFFFFu;
    } else {
        DofSums s[DOF_ROWS];
#pragma unroll
        for (int k = 0; k < DOF_ROWS; k++) s[k].w = s[k].r = s[k].g = s[k].b = 0u;
        for (int32_t dy = -reach; dy <= reach; dy++)
            for (int32_t dx = -reach; dx <= reach; dx++) {
                const uint32_t dist = (uint32_t)max(abs(dx), abs(dy));
                const uint2 *q = own + dy * DOF_LDS_W + dx;
#pragma unroll
                for (int k = 0; k < DOF_ROWS; k++) {
                    const uint2 e = q[k * DOF_LDS_W];
                    dof_tap(s[k], e.x, e.y, dist);
                }
            }
#pragma unroll
        for (int k = 0; k < DOF_ROWS; k++) res[k] = dof_finish(s[k]);
    }
    __syncthreads();  // every tap has been read: the results take the place of the first rows
    uint32_t *s_out = reinterpret_cast<uint32_t *>(s_px);
#pragma unroll
    for (int k = 0; k < DOF_ROWS; k++) s_out[(row0 + k) * TILE_W + col] = res[k];
    __syncthreads();
    if (!share) return;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint4 v = *reinterpret_cast<const uint4 *>(&s_out[srow * TILE_W + (sx - x0) + 4 * k]);
        px[4 * k + 0] = v.x, px[4 * k + 1] = v.y, px[4 * k + 2] = v.z, px[4 * k + 3] = v.w;
    }
    dof_store_share<WIDE>(o, px, n_px);
}

// Bloom (tr_scene_bloom): the frame's highlights keyed, blurred by a fixed tent and added back, into `out`, never in
// place (a tap reads a neighbour's colour); tr_bloom.h has the rule.  One workgroup of 256 lanes per 128 x 16 tile, the
// tiles and colour shares of k_dof.  The tent is a product, so the blur is two passes of 2 R + 1 taps through LDS
// instead of (2 R + 1)^2 taps:
//   * the nine colour flags of the 3 x 3 neighbourhood are workgroup-uniform (a tile outside the grid counts as up).
//     All nine up: the tile is zeros, stored without loading a pixel, ahead of any barrier;
//   * staging: the KEYED tile and a halo of R pixels go to LDS as rows of 160 words (one packed pixel each) that start
//     16 pixels left of the tile, so that a piece of four pixels -- twelve bytes, three aligned words of the frame --
//     lies in ONE tile: a piece in a tile whose flag is up, or outside the frame, is zeros without a load.  16 + 2 R rows;
//   * the vote: whether any staged pixel passed the key (a wave vote and four words of LDS behind the staging
//     barrier).  None: no glow reaches the tile -- it is a copy of its own colour, or zeros under TR_BLOOM_GLOW_ONLY;
//   * the horizontal pass, LDS to LDS: a lane owns one column and every other staged row.  Lanes run along the row, so a
//     tap is 64 consecutive words (ds_read_b32: lane l on bank l % 32 of its half-wave, no conflict) and dx is a loop
//     variable, the weight scalar.  r and b accumulate in the halves of one word (each sum <= 65280 < 2^16), g in a
//     second: u16 sums, as a plane of words {r | b << 16} and a plane of u16 g, rows of 128 behind the staged rows;
//   * the vertical pass, into registers: a lane owns one column and eight of its rows and reads the 8 + 2 R sums of its
//     column once each (64 consecutive words, and 64 consecutive u16 -- two lanes to a word, the same word), adding
//     each to the rows it reaches;
//   * glow: a plain u32 division by D = (R + 1)^4 per channel (24 per lane);
//   * the glow goes through the first 8 KB of the staged rows (nobody reads them after the horizontal pass) to the
//     colour shares -- a lane owns 16 pixels of a row --, which load their own 16 pixels of the frame again (three
//     16-byte loads; none under TR_BLOOM_GLOW_ONLY or behind a raised flag), add and store every byte of the tile;
//   * out_clean, when given, gets the tile's flag: 1 where the tile was stored as zeros on the flags alone, else 0.
// LDS: (16 + 2 R) * (640 + 512 + 256) bytes, dynamic: 25 KB at radius 1, 44 KB at 8, 63.25 KB at 15 (below 64 KB).
// fb and every flag of the frame are only read.  WIDE: width % 16 == 0 and fb and out 16-byte aligned (the launcher
// checks); otherwise the same through byte accesses guarded by the width.  No atomics, no scratch.
constexpr int BLOOM_LDS_W = TILE_W + 32;
constexpr int BLOOM_THREADS = 256, BLOOM_ROWS = TILE_W * TILE_H / BLOOM_THREADS;  // rows of its column a lane owns

// The 16 pixels of a share of the frame (24 bits each) from `q`: three 16-byte pieces, or n_px * 3 guarded bytes.
template <bool WIDE>
__device__ __forceinline__ void bloom_load_share(const uint8_t *q, uint32_t (&px)[16], int32_t n_px)
{
    if (WIDE) {
        uint32_t w[12];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const uint4 v = reinterpret_cast<const uint4 *>(q)[k];
            w[4 * k + 0] = v.x, w[4 * k + 1] = v.y, w[4 * k + 2] = v.z, w[4 * k + 3] = v.w;
        }
#pragma unroll
        for (int g = 0; g < 4; g++) {
            px[4 * g + 0] = w[3 * g] & 0xFFFFFFu;
            px[4 * g + 1] = (w[3 * g] >> 24) | ((w[3 * g + 1] & 0xFFFFu) << 8);
            px[4 * g + 2] = (w[3 * g + 1] >> 16) | ((w[3 * g + 2] & 0xFFu) << 16);
            px[4 * g + 3] = w[3 * g + 2] >> 8;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 16; i++)
            px[i] = i < n_px ? bloom_pack(q[3 * i], q[3 * i + 1], q[3 * i + 2]) : 0u;
    }
}

template <bool WIDE>
__global__ __launch_bounds__(BLOOM_THREADS) void k_bloom(BloomArgs a)
{
    static_assert(TILE_W == 128 && BLOOM_MAX_RADIUS <= 16 && BLOOM_MAX_RADIUS <= TILE_H, "the halo lies in the eight tiles around");
    static_assert(BLOOM_THREADS == 4 * 64 && 8 * TILE_H <= BLOOM_THREADS && BLOOM_THREADS == 2 * TILE_W, "four waves vote; the shares are the first lanes");
    static_assert((TILE_H + 2) * BLOOM_LDS_W >= TILE_H * TILE_W, "the glow of a tile fits the staged rows of radius 1");
    // (TILE_H + 2 R) rows of BLOOM_LDS_W keyed pixels, then as many rows of TILE_W words {r | b << 16}, then of TILE_W u16 g
    extern __shared__ __align__(16) uint32_t s_key[];
    __shared__ uint32_t s_any[4];
    const int32_t W = (int32_t)a.frame.width, H = (int32_t)a.frame.height, R = (int32_t)a.rule.radius;
    const int32_t ntx = (int32_t)a.frame.ntx, nty = (int32_t)a.frame.nty;
    // block b takes the tile of its row ty = b / ntx that lies 5 * ty columns (cyclically) right of column b % ntx.
    // Blocks are dealt round-robin to the XCDs and their shader engines, in order: with 32 tiles to a row (4096
    // pixels) block b % 32 is always the same tile column, and a model in the middle columns loads half of the engines
    // with all the blurred tiles while the rest run the tiles that leave at once (DESIGN 7k has the counters).  A rotation
    // is a permutation of the row for every ntx; it mixes the columns over the engines where 5 and ntx share no factor
    // (every power of two), and is the identity again only for ntx = 5 (and moves within 2 columns for ntx = 10).
    const int32_t ty = (int32_t)blockIdx.x / ntx, tx = ((int32_t)blockIdx.x % ntx + 5 * ty) % ntx;
    const uint32_t t = (uint32_t)(ty * ntx + tx);
    const int32_t x0 = tx * TILE_W, y0 = ty * TILE_H;
    // bit 3 * ay + ax, the tile at (tx + ax - 1, ty + ay - 1): its colour reads as zeros (no such tile, or its flag is up)
    uint32_t czero = 0u;
#pragma unroll
    for (int32_t ay = 0; ay < 3; ay++)
#pragma unroll
        for (int32_t ax = 0; ax < 3; ax++) {
            const int32_t nx = tx + ax - 1, ny = ty + ay - 1;
            const uint32_t bit = 1u << (3 * ay + ax);
            if (nx < 0 || nx >= ntx || ny < 0 || ny >= nty) czero |= bit;
            else if (a.fbclean != nullptr && a.fbclean[ny * ntx + nx] != 0u) czero |= bit;
        }
    const uint32_t own_bit = 1u << 4;
    // the colour shares of k_composite
    const int32_t sx = x0 + (int32_t)(threadIdx.x % 8u) * 16, srow = (int32_t)(threadIdx.x / 8u), sy = y0 + srow;
    const bool share = threadIdx.x < 8u * TILE_H && sx < W && sy < H;
    const int32_t n_px = share ? min(16, W - sx) : 0;  // (WIDE: 16 or none)
    const size_t share_at = share ? ((size_t)(H - 1 - sy) * (size_t)W + (size_t)sx) * 3u : 0u;
    uint8_t *o = a.out + share_at;
    uint32_t px[16];
    const bool all_zero = czero == 0x1FFu;
    if (a.out_clean != nullptr && threadIdx.x == 0u) a.out_clean[t] = all_zero ? 1u : 0u;
    if (all_zero) {  // (workgroup-uniform, ahead of the barriers)
        if (!share) return;
#pragma unroll
        for (int i = 0; i < 16; i++) px[i] = 0u;
        dof_store_share<WIDE>(o, px, n_px);
        return;
    }
    const int32_t rows = TILE_H + 2 * R;  // LDS row r is frame row y0 - R + r, LDS column c frame column x0 - 16 + c
    const uint32_t thr = a.rule.threshold;
    uint32_t passed = 0u;                 // the keyed pixels this lane staged, or-ed
    if (WIDE) {
        for (int32_t p = (int32_t)threadIdx.x; p < rows * (BLOOM_LDS_W / 4); p += BLOOM_THREADS) {
            const int32_t r = p / (BLOOM_LDS_W / 4), j = p % (BLOOM_LDS_W / 4);
            if (4 * j + 3 < 16 - R || 4 * j >= 16 + TILE_W + R) continue;  // (no tap reaches it)
            const int32_t x = x0 - 16 + 4 * j, y = y0 - R + r;
            const int32_t ax = j < 4 ? 0 : j < 4 + TILE_W / 4 ? 1 : 2, ay = y < y0 ? 0 : y < y0 + TILE_H ? 1 : 2;
            const uint32_t bit = 1u << (3 * ay + ax);
            uint32_t c[4] = { 0u, 0u, 0u, 0u };
            if ((czero & bit) == 0u && x < W && y < H) {  // (czero covers the tiles outside the grid: x >= 0 and y >= 0 here)
                // four pixels are twelve bytes at a multiple of four: three aligned words
                const uint32_t *q = reinterpret_cast<const uint32_t *>(a.fb + ((size_t)(H - 1 - y) * (size_t)W + (size_t)x) * 3u);
                const uint32_t w0 = q[0], w1 = q[1], w2 = q[2];
                c[0] = bloom_key(w0 & 0xFFFFFFu, thr);
                c[1] = bloom_key((w0 >> 24) | ((w1 & 0xFFFFu) << 8), thr);
                c[2] = bloom_key((w1 >> 16) | ((w2 & 0xFFu) << 16), thr);
                c[3] = bloom_key(w2 >> 8, thr);
            }
            passed |= c[0] | c[1] | c[2] | c[3];
            *reinterpret_cast<uint4 *>(&s_key[r * BLOOM_LDS_W + 4 * j]) = make_uint4(c[0], c[1], c[2], c[3]);
        }
    } else {
        for (int32_t p = (int32_t)threadIdx.x; p < rows * BLOOM_LDS_W; p += BLOOM_THREADS) {
            const int32_t r = p / BLOOM_LDS_W, c = p % BLOOM_LDS_W;
            if (c < 16 - R || c >= 16 + TILE_W + R) continue;
            const int32_t x = x0 - 16 + c, y = y0 - R + r;
            const int32_t ax = c < 16 ? 0 : c < 16 + TILE_W ? 1 : 2, ay = y < y0 ? 0 : y < y0 + TILE_H ? 1 : 2;
            const uint32_t bit = 1u << (3 * ay + ax);
            uint32_t col = 0u;
            if ((czero & bit) == 0u && x < W && y < H) {
                const uint8_t *q = a.fb + ((size_t)(H - 1 - y) * (size_t)W + (size_t)x) * 3u;
                col = bloom_key(bloom_pack(q[0], q[1], q[2]), thr);
            }
            passed |= col;
            s_key[r * BLOOM_LDS_W + c] = col;
        }
    }
    // (a pixel that passes the key has a channel above the threshold: its packed word is not zero)
    const bool wave_any = __any(passed != 0u) != 0;
    if (threadIdx.x % 64u == 0u) s_any[threadIdx.x / 64u] = wave_any ? 1u : 0u;
    __syncthreads();
    const bool any = __builtin_amdgcn_readfirstlane(s_any[0] | s_any[1] | s_any[2] | s_any[3]) != 0u;
    const bool own_zero = (czero & own_bit) != 0u;
    const bool glow_only = a.rule.glow_only != 0u;
    if (!any) {  // (workgroup-uniform) no glow anywhere in the tile: its own colour, or zeros
        if (!share) return;
#pragma unroll
        for (int i = 0; i < 16; i++) px[i] = 0u;
        if (!glow_only && !own_zero) bloom_load_share<WIDE>(a.fb + share_at, px, n_px);
        dof_store_share<WIDE>(o, px, n_px);
        return;
    }
    // the horizontal pass: column `col`, staged rows half, half + 2, ...
    const int32_t col = (int32_t)threadIdx.x % TILE_W, half = (int32_t)threadIdx.x / TILE_W;
    uint32_t *s_rb = s_key + rows * BLOOM_LDS_W;
    uint16_t *s_g = reinterpret_cast<uint16_t *>(s_rb + rows * TILE_W);
    for (int32_t r = half; r < rows; r += BLOOM_THREADS / TILE_W) {
        const uint32_t *src = s_key + r * BLOOM_LDS_W + 16 + col;
        BloomH h = { 0u, 0u };
        for (int32_t dx = -R; dx <= R; dx++) bloom_h_tap(h, src[dx], bloom_weight(R, dx));
        s_rb[r * TILE_W + col] = h.rb;
        s_g[r * TILE_W + col] = (uint16_t)h.g;
    }
    __syncthreads();
    // the vertical pass: column `col`, rows row0 .. row0 + BLOOM_ROWS - 1 of the tile; staged row row0 + j is dy = j - R - k
    // away from the lane's row k
    const int32_t row0 = half * BLOOM_ROWS;
    BloomV v[BLOOM_ROWS];
#pragma unroll
    for (int k = 0; k < BLOOM_ROWS; k++) v[k].r = v[k].g = v[k].b = 0u;
    for (int32_t j = 0; j < BLOOM_ROWS + 2 * R; j++) {
        const BloomH h = { s_rb[(row0 + j) * TILE_W + col], (uint32_t)s_g[(row0 + j) * TILE_W + col] };
#pragma unroll
        for (int k = 0; k < BLOOM_ROWS; k++) {
            const int32_t w = R + 1 - abs(j - R - k);  // (scalar: j, R and k are)
            bloom_v_tap(v[k], h, (uint32_t)max(w, 0));
        }
    }
    const uint32_t D = bloom_divisor(a.rule.radius);
    uint32_t *s_out = s_key;  // (the staged rows were last read before the barrier above)
#pragma unroll
    for (int k = 0; k < BLOOM_ROWS; k++) s_out[(row0 + k) * TILE_W + col] = bloom_glow_px(v[k], D);
    __syncthreads();
    if (!share) return;
    uint32_t f[16];
#pragma unroll
    for (int i = 0; i < 16; i++) f[i] = 0u;
    if (!glow_only && !own_zero) bloom_load_share<WIDE>(a.fb + share_at, f, n_px);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint4 g = *reinterpret_cast<const uint4 *>(&s_out[srow * TILE_W + (sx - x0) + 4 * k]);
        px[4 * k + 0] = bloom_out_px(f[4 * k + 0], g.x, a.rule);
        px[4 * k + 1] = bloom_out_px(f[4 * k + 1], g.y, a.rule);
        px[4 * k + 2] = bloom_out_px(f[4 * k + 2], g.z, a.rule);
        px[4 * k + 3] = bloom_out_px(f[4 * k + 3], g.w, a.rule);
    }
    dof_store_share<WIDE>(o, px, n_px);
}

// Convolve (tr_scene_convolve): the frame filtered through a kernel of integer weights into `out`, never in place (a tap
// reads a neighbour's colour); tr_convolve.h has the rule.  One workgroup of 256 lanes per 128 x 16 tile, the tiles,
// colour shares and rotated block-to-tile mapping of k_bloom.  The kernel's rows are the buffer's (row 0 = bottom): the
// rule's row j from the top lies ry - j rows ABOVE the pixel, so staged row r feeds the lane's row k with j = k + 2 ry - r.
//   * the nine colour flags of the 3 x 3 neighbourhood are workgroup-uniform.  Every neighbour that exists up, and no
//     border colour in reach (CLAMP, a border of 0, or the halo inside the image): the tile is the constant
//     convolve_of_zeros, stored without a load, ahead of any barrier; out_clean gets 1 only where that constant is 0;
//   * staging: the tile and its halo of rx columns and ry rows go to LDS as rows of 160 words (one packed pixel each)
//     that start 16 pixels left of the tile.  A texel outside the image is the border colour, or under CLAMP the texel at
//     the clamped index (which lies in one of the nine tiles); a texel behind a raised flag is zeros WITHOUT a load --
//     that memory is stale.  a.words: four pixels are twelve bytes, three aligned words of the frame, in one tile;
//   * SEP, the separable form, runs the VERTICAL pass first, LDS to LDS, and the horizontal pass into registers: the
//     tile is 128 x 16, so the vertical sums are 16 rows of 128 + 2 rx columns (30 KB as three int32 planes), where
//     horizontal sums would be 16 + 2 ry rows of 128 (69 KB at 31 taps, beyond the 64 KB a workgroup may ask for).
//     The integers are the same in either order.  A vertical sum is below 255 * sum |col|; M24: that is below 2^23 and
//     the horizontal pass multiplies in 24 bits, otherwise in 32.  A lane owns a column and eight rows in both passes;
//     the eight weights a staged row feeds are a window that slides by one a row: one scalar load a row or a tap;
//   * the general form takes its kw * kh taps from the staged tile, column by column of the kernel, by the same window;
//   * a weight of 0 is skipped by a uniform branch (horizontal pass) or costs its multiply-adds (the windows);
//   * the results go through the first 8 KB of the staged rows to the colour shares -- a lane owns 16 pixels of a row.
// LDS, dynamic: (16 + 2 ry) * 640 bytes, and 30,720 more for SEP: 10 KB at 1 x 1 general, 15 KB at 9 x 9, 58.75 KB at
// 31 x 31.  fb and every flag of the frame are only read.  STORE (the launcher checks): 2 -- width % 16 == 0 and out
// 16-byte aligned, a share is three 16-byte stores; 1 -- width % 4 == 0 and out 4-byte aligned, a share is up to four
// 12-byte pieces; 0 -- guarded bytes.  No atomics, no scratch, no inline assembly.
constexpr int CONV_LDS_W = TILE_W + 32, CONV_THREADS = 256, CONV_ROWS = TILE_W * TILE_H / CONV_THREADS;
static_assert((TILE_H + 2 * (CONVOLVE_MAX_SEPARABLE / 2)) * CONV_LDS_W * 4 + 3 * TILE_H * CONV_LDS_W * 4 < 65536, "the largest kernel's LDS is below 64 KB");
static_assert(CONVOLVE_MAX_SEPARABLE / 2 <= 15 && CONVOLVE_MAX_SEPARABLE / 2 < TILE_H, "the halo lies in the eight tiles around, 16 columns left of the tile included");

// The window of a lane's eight rows over one staged column: `src` is the lane's first staged row (row stride
// CONV_LDS_W), n_rows = CONV_ROWS + 2 ry staged rows feed it, staged row jj feeds row k with the weight
// weights[w0 + (k + 2 ry - jj) * w_stride] where that index is a row of the kernel.
#define CONV_WINDOW(acc, src, w0, w_stride)                                                                          \
    {                                                                                                                \
        int32_t wk[CONV_ROWS];                                                                                       \
        _Pragma("unroll") for (int k = 0; k < CONV_ROWS; k++) wk[k] = 0;                                             \
        wk[0] = a.rule.weights[(w0) + 2 * ry * (w_stride)];                                                          \
        for (int32_t jj = 0; jj < CONV_ROWS + 2 * ry; jj++) {                                                        \
            const int32_t jn = 2 * ry - jj - 1;                                                                      \
            const int32_t w_next = jn >= 0 ? a.rule.weights[(w0) + jn * (w_stride)] : 0;                             \
            const uint32_t px = (src)[jj * CONV_LDS_W];                                                              \
            const int32_t pr = (int32_t)(px & 0xFFu), pg = (int32_t)((px >> 8) & 0xFFu), pb = (int32_t)(px >> 16);   \
            _Pragma("unroll") for (int k = 0; k < CONV_ROWS; k++) {                                                  \
                acc[k][0] += convolve_mul24(wk[k], pr);                                                              \
                acc[k][1] += convolve_mul24(wk[k], pg);                                                              \
                acc[k][2] += convolve_mul24(wk[k], pb);                                                              \
            }                                                                                                        \
            _Pragma("unroll") for (int k = CONV_ROWS - 1; k > 0; k--) wk[k] = wk[k - 1];                             \
            wk[0] = w_next;                                                                                          \
        }                                                                                                            \
    }

// The 16 finished pixels of a share (24 bits each) into `o`.  STORE 2: three 16-byte pieces (k_dof's wide form); 1: a
// piece of four pixels is twelve bytes at a multiple of four -- three words stored together --, n_px / 4 pieces (the
// width is a multiple of 4, so n_px is); 0: n_px * 3 guarded bytes.
template <int STORE>
__device__ __forceinline__ void conv_store_share(uint8_t *o, const uint32_t (&px)[16], int32_t n_px)
{
    if (STORE == 1) {
        struct alignas(4) Piece {
            uint32_t w0, w1, w2;
        };
#pragma unroll
        for (int g = 0; g < 4; g++)
            if (4 * g < n_px) {
                Piece q;
                q.w0 = px[4 * g] | (px[4 * g + 1] << 24);
                q.w1 = (px[4 * g + 1] >> 8) | (px[4 * g + 2] << 16);
                q.w2 = (px[4 * g + 2] >> 16) | (px[4 * g + 3] << 8);
                reinterpret_cast<Piece *>(o)[g] = q;
            }
    } else {
        dof_store_share<STORE == 2>(o, px, n_px);
    }
}

template <bool SEP, int STORE, bool M24>
__global__ __launch_bounds__(CONV_THREADS) void k_convolve(ConvolveArgs a)
{
    static_assert(TILE_W == 128 && CONV_THREADS == 2 * TILE_W && 8 * TILE_H <= CONV_THREADS && CONV_ROWS == 8, "a lane owns a column and eight rows; the shares are the first lanes");
    // (TILE_H + 2 ry) rows of CONV_LDS_W packed pixels; SEP: then three planes of TILE_H rows of CONV_LDS_W int32 sums
    extern __shared__ __align__(16) uint32_t s_cv[];
    const int32_t W = (int32_t)a.frame.width, H = (int32_t)a.frame.height;
    const int32_t kw = (int32_t)a.rule.kw, kh = (int32_t)a.rule.kh, rx = kw / 2, ry = kh / 2;
    const int32_t ntx = (int32_t)a.frame.ntx, nty = (int32_t)a.frame.nty;
    // (k_bloom's mapping: the tile of row ty that lies 5 * ty columns right of column b % ntx)
    const int32_t ty = (int32_t)blockIdx.x / ntx, tx = ((int32_t)blockIdx.x % ntx + 5 * ty) % ntx;
    const uint32_t t = (uint32_t)(ty * ntx + tx);
    const int32_t x0 = tx * TILE_W, y0 = ty * TILE_H;
    // bit 3 * ay + ax, the tile at (tx + ax - 1, ty + ay - 1): exists -- it is part of the grid; czero -- and its flag is up
    uint32_t exists = 0u, czero = 0u;
#pragma unroll
    for (int32_t ay = 0; ay < 3; ay++)
#pragma unroll
        for (int32_t ax = 0; ax < 3; ax++) {
            const int32_t nx = tx + ax - 1, ny = ty + ay - 1;
            const uint32_t bit = 1u << (3 * ay + ax);
            if (nx < 0 || nx >= ntx || ny < 0 || ny >= nty) continue;
            exists |= bit;
            if (a.fbclean != nullptr && a.fbclean[ny * ntx + nx] != 0u) czero |= bit;
        }
    const bool clamp = a.rule.edge == CONVOLVE_CLAMP;
    const bool halo_inside = x0 - rx >= 0 && x0 + TILE_W + rx <= W && y0 - ry >= 0 && y0 + TILE_H + ry <= H;
    const bool constant = czero == exists && (clamp || a.rule.border == 0u || halo_inside);
    // the colour shares of k_composite
    const int32_t sx = x0 + (int32_t)(threadIdx.x % 8u) * 16, srow = (int32_t)(threadIdx.x / 8u), sy = y0 + srow;
    const bool share = threadIdx.x < 8u * TILE_H && sx < W && sy < H;
    const int32_t n_px = share ? min(16, W - sx) : 0;  // (STORE 2: 16 or none; 1: a multiple of 4)
    const size_t share_at = share ? ((size_t)(H - 1 - sy) * (size_t)W + (size_t)sx) * 3u : 0u;
    uint8_t *o = a.out + share_at;
    uint32_t px[16];
    const uint32_t c0 = convolve_of_zeros(a.rule) * 0x010101u;
    if (a.out_clean != nullptr && threadIdx.x == 0u) a.out_clean[t] = constant && c0 == 0u ? 1u : 0u;
    if (constant) {  // (workgroup-uniform, ahead of the barriers)
        if (!share) return;
#pragma unroll
        for (int i = 0; i < 16; i++) px[i] = c0;
        conv_store_share<STORE>(o, px, n_px);
        return;
    }
    // LDS row r is the kernel's row y0 - ry + r, LDS column c the frame's column x0 - 16 + c; columns c_lo .. c_hi - 1 are read
    const int32_t rows = TILE_H + 2 * ry, c_lo = 16 - rx, c_hi = 16 + TILE_W + rx;
    if (a.words != 0u) {
        for (int32_t p = (int32_t)threadIdx.x; p < rows * (CONV_LDS_W / 4); p += CONV_THREADS) {
            const int32_t r = p / (CONV_LDS_W / 4), j = p % (CONV_LDS_W / 4);
            if (4 * j + 3 < c_lo || 4 * j >= c_hi) continue;  // (no tap reaches it)
            const int32_t x = x0 - 16 + 4 * j, y = y0 - ry + r;
            // (x and the width are multiples of 4: the four pixels lie inside the image's columns or outside together)
            const bool x_out = x < 0 || x >= W, y_out = y < 0 || y >= H;
            uint32_t c[4] = { a.rule.border, a.rule.border, a.rule.border, a.rule.border };
            if (clamp || !(x_out || y_out)) {
                const int32_t cx = x < 0 ? 0 : x >= W ? W - 1 : x, cy = y < 0 ? 0 : y >= H ? H - 1 : y;
                const uint32_t bit = 1u << (3 * (cy / TILE_H - ty + 1) + (cx / TILE_W - tx + 1));
                c[0] = c[1] = c[2] = c[3] = 0u;
                if ((czero & bit) == 0u) {
                    const uint8_t *q = a.fb + ((size_t)(H - 1 - cy) * (size_t)W + (size_t)cx) * 3u;
                    if (!x_out) {
                        const uint32_t *q4 = reinterpret_cast<const uint32_t *>(q);
                        const uint32_t w0 = q4[0], w1 = q4[1], w2 = q4[2];
                        c[0] = w0 & 0xFFFFFFu;
                        c[1] = (w0 >> 24) | ((w1 & 0xFFFFu) << 8);
                        c[2] = (w1 >> 16) | ((w2 & 0xFFu) << 16);
                        c[3] = w2 >> 8;
                    } else {
                        c[0] = c[1] = c[2] = c[3] = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16);
                    }
                }
            }
            *reinterpret_cast<uint4 *>(&s_cv[r * CONV_LDS_W + 4 * j]) = make_uint4(c[0], c[1], c[2], c[3]);
        }
    } else {
        for (int32_t p = (int32_t)threadIdx.x; p < rows * CONV_LDS_W; p += CONV_THREADS) {
            const int32_t r = p / CONV_LDS_W, c = p % CONV_LDS_W;
            if (c < c_lo || c >= c_hi) continue;
            const int32_t x = x0 - 16 + c, y = y0 - ry + r;
            uint32_t col = a.rule.border;
            if (clamp || !(x < 0 || x >= W || y < 0 || y >= H)) {
                const int32_t cx = x < 0 ? 0 : x >= W ? W - 1 : x, cy = y < 0 ? 0 : y >= H ? H - 1 : y;
                const uint32_t bit = 1u << (3 * (cy / TILE_H - ty + 1) + (cx / TILE_W - tx + 1));
                col = 0u;
                if ((czero & bit) == 0u) {
                    const uint8_t *q = a.fb + ((size_t)(H - 1 - cy) * (size_t)W + (size_t)cx) * 3u;
                    col = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16);
                }
            }
            s_cv[r * CONV_LDS_W + c] = col;
        }
    }
    __syncthreads();
    const int32_t col = (int32_t)threadIdx.x % TILE_W, row0 = (int32_t)threadIdx.x / TILE_W * CONV_ROWS;
    int32_t acc[CONV_ROWS][3];
#pragma unroll
    for (int k = 0; k < CONV_ROWS; k++) acc[k][0] = acc[k][1] = acc[k][2] = 0;
    if (SEP) {
        // the vertical pass: staged column c, rows 8 h .. 8 h + 7 of the tile, into the planes
        int32_t *s_v = reinterpret_cast<int32_t *>(s_cv + rows * CONV_LDS_W);
        const int32_t n_cols = c_hi - c_lo;
        for (int32_t item = (int32_t)threadIdx.x; item < 2 * n_cols; item += CONV_THREADS) {
            const int32_t h = item >= n_cols ? 1 : 0, c = item - h * n_cols + c_lo;
            int32_t v[CONV_ROWS][3];
#pragma unroll
            for (int k = 0; k < CONV_ROWS; k++) v[k][0] = v[k][1] = v[k][2] = 0;
            const uint32_t *src = s_cv + h * CONV_ROWS * CONV_LDS_W + c;
            CONV_WINDOW(v, src, kw, 1)
#pragma unroll
            for (int k = 0; k < CONV_ROWS; k++)
#pragma unroll
                for (int ch = 0; ch < 3; ch++) s_v[(ch * TILE_H + h * CONV_ROWS + k) * CONV_LDS_W + c] = v[k][ch];
        }
        __syncthreads();
        // the horizontal pass: column `col`, rows row0 .. row0 + 7 of the tile
        for (int32_t i = 0; i < kw; i++) {
            const int32_t w = a.rule.weights[i];
            if (w == 0) continue;  // (scalar)
            const int32_t *src = s_v + row0 * CONV_LDS_W + 16 + col + i - rx;
#pragma unroll
            for (int k = 0; k < CONV_ROWS; k++)
#pragma unroll
                for (int ch = 0; ch < 3; ch++) {
                    const int32_t v = src[(ch * TILE_H + k) * CONV_LDS_W];
                    acc[k][ch] += M24 ? convolve_mul24(w, v) : w * v;
                }
        }
    } else {
        for (int32_t i = 0; i < kw; i++) {
            const uint32_t *src = s_cv + row0 * CONV_LDS_W + 16 + col + i - rx;
            CONV_WINDOW(acc, src, i, kw)
        }
    }
    // the frame's own pixels, staged: row k of the tile is staged row ry + k
    uint32_t res[CONV_ROWS];
#pragma unroll
    for (int k = 0; k < CONV_ROWS; k++)
        res[k] = convolve_finish_px(acc[k][0], acc[k][1], acc[k][2], s_cv[(ry + row0 + k) * CONV_LDS_W + 16 + col], a.rule);
    __syncthreads();  // every staged pixel has been read: the results take the place of the first rows
    uint32_t *s_out = s_cv;
#pragma unroll
    for (int k = 0; k < CONV_ROWS; k++) s_out[(row0 + k) * TILE_W + col] = res[k];
    __syncthreads();
    if (!share) return;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint4 v = *reinterpret_cast<const uint4 *>(&s_out[srow * TILE_W + (sx - x0) + 4 * k]);
        px[4 * k + 0] = v.x, px[4 * k + 1] = v.y, px[4 * k + 2] = v.z, px[4 * k + 3] = v.w;
    }
    conv_store_share<STORE>(o, px, n_px);
}
#undef CONV_WINDOW

// Rank (tr_scene_rank): the frame through an order-statistic filter over a footprint of taps into `out`, never in place;
// tr_rank.h has the rule.  The tile, the workgroup, the rotated block-to-tile mapping, the nine-flag test, the staged
// rows of 160 words that start 16 pixels left of the tile, the window of a lane's eight rows over a staged column and
// the three store forms are k_convolve's.  What differs:
//   * a neighbourhood of zeros is 0 under every op: the constant tile is zeros and out_clean gets 1;
//   * a staged pixel is SPREAD, r | g << 10 | b << 20, so that one subtraction compares three channels at once: with
//     bit 9 of every field set in p, field c of p - t is 512 + p_c - t_c, and its bit 9 says p_c >= t_c (no field
//     borrows from its neighbour: 257 <= 512 + p_c - t_c <= 767);
//   * SEL 0, any rank of any footprint: eight steps from bit 7 down build v(k) a channel -- the candidate t | bit stays
//     where the number of taps below it is at most k, that is where ge, the number of taps at or above it, is at least
//     n - k.  ge of three channels is one word of 10-bit fields (n <= 225), the test against n - k the same subtraction.
//     A staged value feeds the eight windows of the lane; whether row j, column i of the box is a tap is a scalar, the
//     window of eight such scalars slides by one a staged row; a column of the box without a tap is skipped.  An op of
//     two ranks searches twice;
//   * SEL 1, 2, 3, the extremes: every rank asked for is 0 or n - 1, so no selection -- the minimum (bit 0 of SEL)
//     and/or the maximum (bit 1) over the taps, one pass; a pixel outside the footprint enters as 255 or as 0.
// LDS, dynamic: (16 + 2 ry) * 640 bytes, 10 KB at a box one row high, 19.2 KB at fifteen.  fb and every flag of the
// frame are only read.  No atomics, no scratch, no inline assembly.
constexpr uint32_t RANK_ONES = 0x00100401u, RANK_HIGH = RANK_ONES << 9;
static_assert(RANK_MAX_TAPS < 512u && RANK_MAX_SIDE / 2u <= 15u && (int)(RANK_MAX_SIDE / 2u) < TILE_H, "a count fits a 10-bit field; the halo lies in the eight tiles around");

__device__ __forceinline__ uint32_t rank_spread(uint32_t px) { return (px & 0xFFu) | ((px & 0xFF00u) << 2) | ((px & 0xFF0000u) << 4); }
__device__ __forceinline__ uint32_t rank_unspread(uint32_t v) { return (v & 0xFFu) | ((v >> 2) & 0xFF00u) | ((v >> 4) & 0xFF0000u); }

// Is column i of row j (from the top) a tap, for a row index that may lie outside the box?  (scalar)
__device__ __forceinline__ uint32_t rank_member(const RankArgs &a, int32_t i, int32_t j, int32_t kh)
{
    return j >= 0 && j < kh ? (a.rule.rows[j] >> i) & 1u : 0u;
}

// v(k) of the lane's eight windows, spread: `src` is the lane's first staged row at the column of the box's column 0.
__device__ __forceinline__ void rank_search(const uint32_t *src, const RankArgs &a, uint32_t k, uint32_t col_mask, uint32_t (&t)[CONV_ROWS])
{
    const int32_t kw = (int32_t)a.rule.kw, kh = (int32_t)a.rule.kh, ry = kh / 2;
    const uint32_t need = (a.rule.n - k) * RANK_ONES;
#pragma unroll
    for (int r = 0; r < CONV_ROWS; r++) t[r] = 0u;
    for (int32_t b = 7; b >= 0; b--) {
        uint32_t cand[CONV_ROWS], ge[CONV_ROWS];
#pragma unroll
        for (int r = 0; r < CONV_ROWS; r++) cand[r] = t[r] | (RANK_ONES << b), ge[r] = 0u;
        for (int32_t i = 0; i < kw; i++) {
            if (((col_mask >> i) & 1u) == 0u) continue;  // (scalar)
            uint32_t wk[CONV_ROWS];
#pragma unroll
            for (int r = 0; r < CONV_ROWS; r++) wk[r] = 0u;
            wk[0] = rank_member(a, i, 2 * ry, kh) * RANK_ONES;
            for (int32_t jj = 0; jj < CONV_ROWS + 2 * ry; jj++) {
                const uint32_t w_next = rank_member(a, i, 2 * ry - jj - 1, kh) * RANK_ONES;
                const uint32_t p = src[jj * CONV_LDS_W + i] | RANK_HIGH;
#pragma unroll
                for (int r = 0; r < CONV_ROWS; r++) ge[r] += ((p - cand[r]) >> 9) & wk[r];
#pragma unroll
                for (int r = CONV_ROWS - 1; r > 0; r--) wk[r] = wk[r - 1];
                wk[0] = w_next;
            }
        }
#pragma unroll
        for (int r = 0; r < CONV_ROWS; r++) t[r] |= ((((ge[r] | RANK_HIGH) - need) >> 9) & RANK_ONES) << b;
    }
}

template <int SEL, int STORE>
__global__ __launch_bounds__(CONV_THREADS) void k_rank(RankArgs a)
{
    static_assert(TILE_W == 128 && CONV_THREADS == 2 * TILE_W && 8 * TILE_H <= CONV_THREADS && CONV_ROWS == 8, "a lane owns a column and eight rows; the shares are the first lanes");
    extern __shared__ __align__(16) uint32_t s_rk[];  // (TILE_H + 2 ry) rows of CONV_LDS_W spread pixels
    const int32_t W = (int32_t)a.frame.width, H = (int32_t)a.frame.height;
    const int32_t kw = (int32_t)a.rule.kw, kh = (int32_t)a.rule.kh, rx = kw / 2, ry = kh / 2;
    const int32_t ntx = (int32_t)a.frame.ntx, nty = (int32_t)a.frame.nty;
    const int32_t ty = (int32_t)blockIdx.x / ntx, tx = ((int32_t)blockIdx.x % ntx + 5 * ty) % ntx;
    const uint32_t t = (uint32_t)(ty * ntx + tx);
    const int32_t x0 = tx * TILE_W, y0 = ty * TILE_H;
    // bit 3 * ay + ax, the tile at (tx + ax - 1, ty + ay - 1): exists -- it is part of the grid; czero -- and its flag is up
    uint32_t exists = 0u, czero = 0u;
#pragma unroll
    for (int32_t ay = 0; ay < 3; ay++)
#pragma unroll
        for (int32_t ax = 0; ax < 3; ax++) {
            const int32_t nx = tx + ax - 1, ny = ty + ay - 1;
            const uint32_t bit = 1u << (3 * ay + ax);
            if (nx < 0 || nx >= ntx || ny < 0 || ny >= nty) continue;
            exists |= bit;
            if (a.fbclean != nullptr && a.fbclean[ny * ntx + nx] != 0u) czero |= bit;
        }
    const bool clamp = a.rule.edge == RANK_CLAMP;
    const bool halo_inside = x0 - rx >= 0 && x0 + TILE_W + rx <= W && y0 - ry >= 0 && y0 + TILE_H + ry <= H;
    const bool constant = czero == exists && (clamp || a.rule.border == 0u || halo_inside);
    const int32_t sx = x0 + (int32_t)(threadIdx.x % 8u) * 16, srow = (int32_t)(threadIdx.x / 8u), sy = y0 + srow;
    const bool share = threadIdx.x < 8u * TILE_H && sx < W && sy < H;
    const int32_t n_px = share ? min(16, W - sx) : 0;  // (STORE 2: 16 or none; 1: a multiple of 4)
    const size_t share_at = share ? ((size_t)(H - 1 - sy) * (size_t)W + (size_t)sx) * 3u : 0u;
    uint8_t *o = a.out + share_at;
    uint32_t px[16];
    if (a.out_clean != nullptr && threadIdx.x == 0u) a.out_clean[t] = constant ? 1u : 0u;
    if (constant) {  // (workgroup-uniform, ahead of the barriers)
        if (!share) return;
#pragma unroll
        for (int i = 0; i < 16; i++) px[i] = 0u;
        conv_store_share<STORE>(o, px, n_px);
        return;
    }
    // LDS row r is the kernel's row y0 - ry + r, LDS column c the frame's column x0 - 16 + c; columns c_lo .. c_hi - 1 are read
    const int32_t rows = TILE_H + 2 * ry, c_lo = 16 - rx, c_hi = 16 + TILE_W + rx;
    const uint32_t border = rank_spread(a.rule.border);
    if (a.words != 0u) {
        for (int32_t p = (int32_t)threadIdx.x; p < rows * (CONV_LDS_W / 4); p += CONV_THREADS) {
            const int32_t r = p / (CONV_LDS_W / 4), j = p % (CONV_LDS_W / 4);
            if (4 * j + 3 < c_lo || 4 * j >= c_hi) continue;  // (no tap reaches it)
            const int32_t x = x0 - 16 + 4 * j, y = y0 - ry + r;
            // (x and the width are multiples of 4: the four pixels lie inside the image's columns or outside together)
            const bool x_out = x < 0 || x >= W, y_out = y < 0 || y >= H;
            uint32_t c[4] = { border, border, border, border };
            if (clamp || !(x_out || y_out)) {
                const int32_t cx = x < 0 ? 0 : x >= W ? W - 1 : x, cy = y < 0 ? 0 : y >= H ? H - 1 : y;
                const uint32_t bit = 1u << (3 * (cy / TILE_H - ty + 1) + (cx / TILE_W - tx + 1));
                c[0] = c[1] = c[2] = c[3] = 0u;
                if ((czero & bit) == 0u) {
                    const uint8_t *q = a.fb + ((size_t)(H - 1 - cy) * (size_t)W + (size_t)cx) * 3u;
                    if (!x_out) {
                        const uint32_t *q4 = reinterpret_cast<const uint32_t *>(q);
                        const uint32_t w0 = q4[0], w1 = q4[1], w2 = q4[2];
                        c[0] = rank_spread(w0 & 0xFFFFFFu);
                        c[1] = rank_spread((w0 >> 24) | ((w1 & 0xFFFFu) << 8));
                        c[2] = rank_spread((w1 >> 16) | ((w2 & 0xFFu) << 16));
                        c[3] = rank_spread(w2 >> 8);
                    } else {
                        c[0] = c[1] = c[2] = c[3] = (uint32_t)q[0] | ((uint32_t)q[1] << 10) | ((uint32_t)q[2] << 20);
                    }
                }
            }
            *reinterpret_cast<uint4 *>(&s_rk[r * CONV_LDS_W + 4 * j]) = make_uint4(c[0], c[1], c[2], c[3]);
        }
    } else {
        for (int32_t p = (int32_t)threadIdx.x; p < rows * CONV_LDS_W; p += CONV_THREADS) {
            const int32_t r = p / CONV_LDS_W, c = p % CONV_LDS_W;
            if (c < c_lo || c >= c_hi) continue;
            const int32_t x = x0 - 16 + c, y = y0 - ry + r;
            uint32_t col = border;
            if (clamp || !(x < 0 || x >= W || y < 0 || y >= H)) {
                const int32_t cx = x < 0 ? 0 : x >= W ? W - 1 : x, cy = y < 0 ? 0 : y >= H ? H - 1 : y;
                const uint32_t bit = 1u << (3 * (cy / TILE_H - ty + 1) + (cx / TILE_W - tx + 1));
                col = 0u;
                if ((czero & bit) == 0u) {
                    const uint8_t *q = a.fb + ((size_t)(H - 1 - cy) * (size_t)W + (size_t)cx) * 3u;
                    col = (uint32_t)q[0] | ((uint32_t)q[1] << 10) | ((uint32_t)q[2] << 20);
                }
            }
            s_rk[r * CONV_LDS_W + c] = col;
        }
    }
    __syncthreads();
    const int32_t col = (int32_t)threadIdx.x % TILE_W, row0 = (int32_t)threadIdx.x / TILE_W * CONV_ROWS;
    // the lane's first staged row at the column of the box's column 0
    const uint32_t *src = s_rk + row0 * CONV_LDS_W + 16 + col - rx;
    uint32_t col_mask = 0u;  // the columns of the box that hold a tap
    for (int32_t j = 0; j < kh; j++) col_mask |= a.rule.rows[j];
    uint32_t lo[CONV_ROWS], hi[CONV_ROWS];  // v(rank), v(rank2), spread
    if (SEL == 0) {
        rank_search(src, a, a.rule.rank, col_mask, lo);
        if (a.rule.rank2 != a.rule.rank) {  // (scalar)
            rank_search(src, a, a.rule.rank2, col_mask, hi);
        } else {
#pragma unroll
            for (int r = 0; r < CONV_ROWS; r++) hi[r] = lo[r];
        }
    } else {
        uint32_t mn[CONV_ROWS][3], mx[CONV_ROWS][3];
#pragma unroll
        for (int r = 0; r < CONV_ROWS; r++) mn[r][0] = mn[r][1] = mn[r][2] = 255u, mx[r][0] = mx[r][1] = mx[r][2] = 0u;
        for (int32_t i = 0; i < kw; i++) {
            if (((col_mask >> i) & 1u) == 0u) continue;  // (scalar)
            uint32_t wk[CONV_ROWS];  // 255 where the staged row is a tap of the lane's row r
#pragma unroll
            for (int r = 0; r < CONV_ROWS; r++) wk[r] = 0u;
            wk[0] = rank_member(a, i, 2 * ry, kh) * 255u;
            for (int32_t jj = 0; jj < CONV_ROWS + 2 * ry; jj++) {
                const uint32_t w_next = rank_member(a, i, 2 * ry - jj - 1, kh) * 255u;
                const uint32_t p = src[jj * CONV_LDS_W + i];
                const uint32_t pc[3] = { p & 0xFFu, (p >> 10) & 0xFFu, p >> 20 };
#pragma unroll
                for (int r = 0; r < CONV_ROWS; r++)
#pragma unroll
                    for (int ch = 0; ch < 3; ch++) {
                        if ((SEL & 1) != 0) mn[r][ch] = min(mn[r][ch], pc[ch] | (wk[r] ^ 255u));
                        if ((SEL & 2) != 0) mx[r][ch] = max(mx[r][ch], pc[ch] & wk[r]);
                    }
#pragma unroll
                for (int r = CONV_ROWS - 1; r > 0; r--) wk[r] = wk[r - 1];
                wk[0] = w_next;
            }
        }
        const bool lo_min = a.rule.rank == 0u, hi_min = a.rule.rank2 == 0u;  // (n = 1: rank 0 is n - 1 too, and the minimum is it)
#pragma unroll
        for (int r = 0; r < CONV_ROWS; r++) {
            const uint32_t vmin = mn[r][0] | (mn[r][1] << 10) | (mn[r][2] << 20), vmax = mx[r][0] | (mx[r][1] << 10) | (mx[r][2] << 20);
            lo[r] = (SEL & 2) == 0 || ((SEL & 1) != 0 && lo_min) ? vmin : vmax;
            hi[r] = (SEL & 2) == 0 || ((SEL & 1) != 0 && hi_min) ? vmin : vmax;
        }
    }
    // the frame's own pixels, staged: row r of the tile is staged row ry + r
    uint32_t res[CONV_ROWS];
#pragma unroll
    for (int r = 0; r < CONV_ROWS; r++)
        res[r] = rank_finish_px(a.rule.op, rank_unspread(lo[r]), rank_unspread(hi[r]), rank_unspread(s_rk[(ry + row0 + r) * CONV_LDS_W + 16 + col]));
    __syncthreads();  // every staged pixel has been read: the results take the place of the first rows
    uint32_t *s_out = s_rk;
#pragma unroll
    for (int r = 0; r < CONV_ROWS; r++) s_out[(row0 + r) * TILE_W + col] = res[r];
    __syncthreads();
    if (!share) return;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint4 v = *reinterpret_cast<const uint4 *>(&s_out[srow * TILE_W + (sx - x0) + 4 * k]);
        px[4 * k + 0] = v.x, px[4 * k + 1] = v.y, px[4 * k + 2] = v.z, px[4 * k + 3] = v.w;
    }
    conv_store_share<STORE>(o, px, n_px);
}

// Bilateral (tr_scene_bilateral): the frame through a weighted mean whose weights fall with a tap's distance from the
// centre, in colour (GUIDE 0) or in depth (GUIDE 1), into `out`, never in place; tr_bilateral.h has the rule.  The tile,
// the workgroup, the rotated block-to-tile mapping, the nine-flag test, the staged rows of 160 words that start 16 pixels
// left of the tile (one packed pixel each, as k_convolve stages them), the window of a lane's eight rows over a staged
// column and the three store forms are k_convolve's; the colour staging is neigh_stage_colour below.  What differs:
//   * a weighted mean of zeros is 0, and S == 0 gives the centre, which is 0 too: the constant tile is zeros under both
//     guides and out_clean gets 1; on that path no depth is loaded;
//   * GUIDE 1 stages z as a second plane of the same rows and halo, element by element (z: x + y * W for the kernel's
//     row y).  A z texel is f32::MIN WITHOUT a load behind a raised depth flag (that memory is stale), outside the image
//     under BORDER, and in a tile outside the grid (k_ao's form; under CLAMP the clamped index lies in the grid);
//   * the range table is 256 bytes of LDS behind the planes, one word a lane of the first wave, staged once: its 64
//     words lie in 64 different banks, a lookup is one byte read at a per-lane index;
//   * the tap loop: a staged pixel (and depth) is read once from LDS and serves the lane's eight centres; the spatial
//     weight of staged row jj for the lane's row k is a scalar, the eight of them a window that slides by one a row; a
//     zero weight -- outside the window or in it -- is skipped by a uniform branch.  S and the three A_c of a centre
//     are u32 (tr_bilateral.h has the bounds), the products 24-bit multiplies;
//   * the finish is a plain u32 division per pixel and channel.
// LDS, dynamic: (16 + 2 ry) * 640 bytes of colour, as much again for z under GUIDE 1, and 256 for the table: 10.25 KB at
// a window one row high under GUIDE 0, 37.75 KB at fifteen rows under GUIDE 1.  fb, z and every flag of the frame are
// only read.  No atomics, no scratch, no inline assembly.
static_assert(BILATERAL_MAX_SIDE / 2u <= 15u && (int)(BILATERAL_MAX_SIDE / 2u) < TILE_H, "the halo lies in the eight tiles around");
static_assert(2 * (TILE_H + 2 * (int)(BILATERAL_MAX_SIDE / 2u)) * CONV_LDS_W * 4 + 256 < 40 * 1024, "the largest window's LDS is below 40 KB");

// The colour staging of a neighbourhood stage, k_convolve's and k_rank's text in one place (k_bilateral calls it; the two
// older kernels keep their own copies: on shared helpers they measured slower than on these): the tile at (x0, y0) =
// (tx, ty) and its halo of rx columns and ry rows into s_px as rows of CONV_LDS_W packed pixels (r | g << 8 | b << 16)
// that start 16 pixels left of the tile.  A texel outside the image is `border`, or under `clamp` the texel at the
// clamped index; a texel behind a raised flag (czero: bit 3 * ay + ax of the 3 x 3 tiles around) is zeros WITHOUT a load.
// words: fb is 4-byte aligned and the width a multiple of 4 -- four pixels are three aligned words.  No barrier here.
__device__ __forceinline__ void neigh_stage_colour(uint32_t *s_px, const uint8_t *fb, bool words, bool clamp, uint32_t border, uint32_t czero, int32_t W, int32_t H,
                                                   int32_t x0, int32_t y0, int32_t tx, int32_t ty, int32_t rx, int32_t ry)
{
    // LDS row r is the kernel's row y0 - ry + r, LDS column c the frame's column x0 - 16 + c; columns c_lo .. c_hi - 1 are read
    const int32_t rows = TILE_H + 2 * ry, c_lo = 16 - rx, c_hi = 16 + TILE_W + rx;
    if (words) {
        for (int32_t p = (int32_t)threadIdx.x; p < rows * (CONV_LDS_W / 4); p += CONV_THREADS) {
            const int32_t r = p / (CONV_LDS_W / 4), j = p % (CONV_LDS_W / 4);
            if (4 * j + 3 < c_lo || 4 * j >= c_hi) continue;  // (no tap reaches it)
            const int32_t x = x0 - 16 + 4 * j, y = y0 - ry + r;
            // (x and the width are multiples of 4: the four pixels lie inside the image's columns or outside together)
            const bool x_out = x < 0 || x >= W, y_out = y < 0 || y >= H;
            uint32_t c[4] = { border, border, border, border };
            if (clamp || !(x_out || y_out)) {
                const int32_t cx = x < 0 ? 0 : x >= W ? W - 1 : x, cy = y < 0 ? 0 : y >= H ? H - 1 : y;
                const uint32_t bit = 1u << (3 * (cy / TILE_H - ty + 1) + (cx / TILE_W - tx + 1));
                c[0] = c[1] = c[2] = c[3] = 0u;
                if ((czero & bit) == 0u) {
                    const uint8_t *q = fb + ((size_t)(H - 1 - cy) * (size_t)W + (size_t)cx) * 3u;
                    if (!x_out) {
                        const uint32_t *q4 = reinterpret_cast<const uint32_t *>(q);
                        const uint32_t w0 = q4[0], w1 = q4[1], w2 = q4[2];
                        c[0] = w0 & 0xFFFFFFu;
                        c[1] = (w0 >> 24) | ((w1 & 0xFFFFu) << 8);
                        c[2] = (w1 >> 16) | ((w2 & 0xFFu) << 16);
                        c[3] = w2 >> 8;
                    } else {
                        c[0] = c[1] = c[2] = c[3] = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16);
                    }
                }
            }
            *reinterpret_cast<uint4 *>(&s_px[r * CONV_LDS_W + 4 * j]) = make_uint4(c[0], c[1], c[2], c[3]);
        }
    } else {
        for (int32_t p = (int32_t)threadIdx.x; p < rows * CONV_LDS_W; p += CONV_THREADS) {
            const int32_t r = p / CONV_LDS_W, c = p % CONV_LDS_W;
            if (c < c_lo || c >= c_hi) continue;
            const int32_t x = x0 - 16 + c, y = y0 - ry + r;
            uint32_t col = border;
            if (clamp || !(x < 0 || x >= W || y < 0 || y >= H)) {
                const int32_t cx = x < 0 ? 0 : x >= W ? W - 1 : x, cy = y < 0 ? 0 : y >= H ? H - 1 : y;
                const uint32_t bit = 1u << (3 * (cy / TILE_H - ty + 1) + (cx / TILE_W - tx + 1));
                col = 0u;
                if ((czero & bit) == 0u) {
                    const uint8_t *q = fb + ((size_t)(H - 1 - cy) * (size_t)W + (size_t)cx) * 3u;
                    col = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16);
                }
            }
            s_px[r * CONV_LDS_W + c] = col;
        }
    }
}

// The spatial weight of column i, row j (from the top) of the window, for a row index that may lie outside it.  (scalar)
__device__ __forceinline__ uint32_t bilateral_spatial(const BilateralArgs &a, int32_t i, int32_t j, int32_t kw, int32_t kh)
{
    return j >= 0 && j < kh ? bilateral_byte(a.rule.spatial, (uint32_t)(j * kw + i)) : 0u;
}

template <int GUIDE, int STORE>
__global__ __launch_bounds__(CONV_THREADS) void k_bilateral(BilateralArgs a)
{
    static_assert(TILE_W == 128 && CONV_THREADS == 2 * TILE_W && 8 * TILE_H <= CONV_THREADS && CONV_ROWS == 8, "a lane owns a column and eight rows; the shares are the first lanes");
    // (TILE_H + 2 ry) rows of CONV_LDS_W packed pixels; GUIDE 1: then as many rows of depths; then the 64 words of the range table
    extern __shared__ __align__(16) uint32_t s_bl[];
    const int32_t W = (int32_t)a.frame.width, H = (int32_t)a.frame.height;
    const int32_t kw = (int32_t)a.rule.kw, kh = (int32_t)a.rule.kh, rx = kw / 2, ry = kh / 2;
    const int32_t ntx = (int32_t)a.frame.ntx, nty = (int32_t)a.frame.nty;
    const int32_t ty = (int32_t)blockIdx.x / ntx, tx = ((int32_t)blockIdx.x % ntx + 5 * ty) % ntx;
    const uint32_t t = (uint32_t)(ty * ntx + tx);
    const int32_t x0 = tx * TILE_W, y0 = ty * TILE_H;
    // bit 3 * ay + ax, the tile at (tx + ax - 1, ty + ay - 1): exists -- it is part of the grid; czero -- and its flag is up
    uint32_t exists = 0u, czero = 0u;
#pragma unroll
    for (int32_t ay = 0; ay < 3; ay++)
#pragma unroll
        for (int32_t ax = 0; ax < 3; ax++) {
            const int32_t nx = tx + ax - 1, ny = ty + ay - 1;
            const uint32_t bit = 1u << (3 * ay + ax);
            if (nx < 0 || nx >= ntx || ny < 0 || ny >= nty) continue;
            exists |= bit;
            if (a.fbclean != nullptr && a.fbclean[ny * ntx + nx] != 0u) czero |= bit;
        }
    const bool clamp = a.rule.edge == BILATERAL_CLAMP;
    const bool halo_inside = x0 - rx >= 0 && x0 + TILE_W + rx <= W && y0 - ry >= 0 && y0 + TILE_H + ry <= H;
    const bool constant = czero == exists && (clamp || a.rule.border == 0u || halo_inside);
    const int32_t sx = x0 + (int32_t)(threadIdx.x % 8u) * 16, srow = (int32_t)(threadIdx.x / 8u), sy = y0 + srow;
    const bool share = threadIdx.x < 8u * TILE_H && sx < W && sy < H;
    const int32_t n_px = share ? min(16, W - sx) : 0;  // (STORE 2: 16 or none; 1: a multiple of 4)
    const size_t share_at = share ? ((size_t)(H - 1 - sy) * (size_t)W + (size_t)sx) * 3u : 0u;
    uint8_t *o = a.out + share_at;
    uint32_t px[16];
    if (a.out_clean != nullptr && threadIdx.x == 0u) a.out_clean[t] = constant ? 1u : 0u;
    if (constant) {  // (workgroup-uniform, ahead of the barriers and of any load of colour or depth)
        if (!share) return;
#pragma unroll
        for (int i = 0; i < 16; i++) px[i] = 0u;
        conv_store_share<STORE>(o, px, n_px);
        return;
    }
    // LDS row r is the kernel's row y0 - ry + r, LDS column c the frame's column x0 - 16 + c; columns c_lo .. c_hi - 1 are read
    const int32_t rows = TILE_H + 2 * ry, c_lo = 16 - rx, c_hi = 16 + TILE_W + rx;
    float *s_z = reinterpret_cast<float *>(s_bl + rows * CONV_LDS_W);
    uint32_t *s_range = s_bl + (GUIDE == 1 ? 2 : 1) * rows * CONV_LDS_W;
    if (threadIdx.x < 64u) s_range[threadIdx.x] = a.rule.range[threadIdx.x];
    neigh_stage_colour(s_bl, a.fb, a.words != 0u, clamp, a.rule.border, czero, W, H, x0, y0, tx, ty, rx, ry);
    if (GUIDE == 1) {
        // bit 3 * ay + ax: the z of that tile reads as f32::MIN -- its depth flag is up, or there is no such tile
        uint32_t zstale = exists ^ 0x1FFu;
#pragma unroll
        for (int32_t ay = 0; ay < 3; ay++)
#pragma unroll
            for (int32_t ax = 0; ax < 3; ax++) {
                const uint32_t bit = 1u << (3 * ay + ax);
                if ((exists & bit) != 0u && a.zclean != nullptr && a.zclean[(ty + ay - 1) * ntx + (tx + ax - 1)] != 0u) zstale |= bit;
            }
        const float z_min = bits_f32(TR_F32_MIN_BITS);
        for (int32_t p = (int32_t)threadIdx.x; p < rows * CONV_LDS_W; p += CONV_THREADS) {
            const int32_t r = p / CONV_LDS_W, c = p % CONV_LDS_W;
            if (c < c_lo || c >= c_hi) continue;
            const int32_t x = x0 - 16 + c, y = y0 - ry + r;
            float v = z_min;
            if (clamp || !(x < 0 || x >= W || y < 0 || y >= H)) {
                const int32_t cx = x < 0 ? 0 : x >= W ? W - 1 : x, cy = y < 0 ? 0 : y >= H ? H - 1 : y;
                const uint32_t bit = 1u << (3 * (cy / TILE_H - ty + 1) + (cx / TILE_W - tx + 1));
                if ((zstale & bit) == 0u) v = a.z[(size_t)cy * (size_t)W + (size_t)cx];
            }
            s_z[r * CONV_LDS_W + c] = v;
        }
    }
    __syncthreads();
    const int32_t col = (int32_t)threadIdx.x % TILE_W, row0 = (int32_t)threadIdx.x / TILE_W * CONV_ROWS;
    const uint8_t *s_rt = reinterpret_cast<const uint8_t *>(s_range);
    // the lane's eight centres, staged: row k of the tile is staged row ry + k
    uint32_t centre[CONV_ROWS];
    float zc[CONV_ROWS];
    BilateralSums m[CONV_ROWS];
#pragma unroll
    for (int k = 0; k < CONV_ROWS; k++) {
        centre[k] = s_bl[(ry + row0 + k) * CONV_LDS_W + 16 + col];
        zc[k] = GUIDE == 1 ? s_z[(ry + row0 + k) * CONV_LDS_W + 16 + col] : 0.0f;
        m[k].s = m[k].a[0] = m[k].a[1] = m[k].a[2] = 0u;
    }
    for (int32_t i = 0; i < kw; i++) {
        // the lane's first staged row at the column of the window's column i
        const int32_t at = row0 * CONV_LDS_W + 16 + col + i - rx;
        uint32_t wk[CONV_ROWS];  // the spatial weight of the staged row for the lane's row k: row k + 2 ry - jj of the window
#pragma unroll
        for (int k = 0; k < CONV_ROWS; k++) wk[k] = 0u;
        wk[0] = bilateral_spatial(a, i, 2 * ry, kw, kh);
        for (int32_t jj = 0; jj < CONV_ROWS + 2 * ry; jj++) {
            const uint32_t w_next = bilateral_spatial(a, i, 2 * ry - jj - 1, kw, kh);
            const uint32_t tp = s_bl[at + jj * CONV_LDS_W];
            const float zt = GUIDE == 1 ? s_z[at + jj * CONV_LDS_W] : 0.0f;
#pragma unroll
            for (int k = 0; k < CONV_ROWS; k++) {
                if (wk[k] == 0u) continue;  // (scalar)
                const uint32_t d = GUIDE == 1 ? bilateral_depth_distance(zt, zc[k], a.rule.depth_scale) : bilateral_colour_distance(tp, centre[k]);
                bilateral_tap(m[k], mul24(wk[k], (uint32_t)s_rt[d]), tp);
            }
#pragma unroll
            for (int k = CONV_ROWS - 1; k > 0; k--) wk[k] = wk[k - 1];
            wk[0] = w_next;
        }
    }
    uint32_t res[CONV_ROWS];
#pragma unroll
    for (int k = 0; k < CONV_ROWS; k++) res[k] = bilateral_finish_px(m[k], centre[k]);
    __syncthreads();  // every staged pixel has been read: the results take the place of the first rows
    uint32_t *s_out = s_bl;
#pragma unroll
    for (int k = 0; k < CONV_ROWS; k++) s_out[(row0 + k) * TILE_W + col] = res[k];
    __syncthreads();
    if (!share) return;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint4 v = *reinterpret_cast<const uint4 *>(&s_out[srow * TILE_W + (sx - x0) + 4 * k]);
        px[4 * k + 0] = v.x, px[4 * k + 1] = v.y, px[4 * k + 2] = v.z, px[4 * k + 3] = v.w;
    }
    conv_store_share<STORE>(o, px, n_px);
}

// Colour grading (tr_scene_grade): every pixel of the frame mapped through the scene's 3-D lookup table into `out`,
// which may BE the frame (a pixel depends on itself alone); tr_grade.h has the rule.  The working set is the table, not
// a neighbourhood, so the workgroups are PERSISTENT: the launcher starts as many as the machine holds at once (by the
// table's LDS size, never more than there are tiles), each stages the table once and then walks the 128 x 16 tiles of
// the scene's grid (a band scene's: its band's) with the stride of the grid, G.
//   * LDS form (N <= 25, at most 62,512 bytes of dynamic LDS): the table is copied from global memory in 16-byte pieces
//     at the first tile the workgroup has to read -- a workgroup whose tiles all leave on their flags never stages it;
//     global form (N = 26..33, up to 144 KB): the four entries of a pixel are gathered from global memory (L2);
//   * which tile: slot k = b, b + G, b + 2 G, ... is row ty = k / ntx of the grid and the column that lies
//     5 * ty + 13 * (ty * ntx / G) columns (cyclically) right of k % ntx -- a function of ty alone, so a permutation of
//     every row whatever G is.  The first term is k_bloom's: a model's tile columns spread over the shader engines.
//     The second moves a workgroup to another column each time it comes round (G is usually a multiple of ntx, and
//     then ty * ntx / G is the round), so every workgroup gets drawn and empty tiles alike;
//   * a tile whose colour-clean flag is up is not read (the flag is workgroup-uniform, one scalar word): it holds
//     zeros and becomes c0, the table's entry 0.  In place with c0 = 0 it is left alone, flag and all; otherwise the
//     constant is stored, and in place lane 0 lowers the flag behind a barrier (every wave has read it by then);
//   * a unit is four pixels of a row, twelve bytes; a lane takes two units of a tile, eight rows apart, and 32 lanes run
//     along a row (384 consecutive bytes).  WORDS: width % 4 == 0 and fb and out 4-byte aligned (the launcher checks),
//     so a unit is three aligned words, loaded and stored as one 12-byte piece; otherwise guarded bytes, which also serve
//     rows whose byte offset is no multiple of 4 (width 130: 390-byte rows).  A lane has read its bytes before it
//     writes them and no other lane touches them: in place is safe.  Rows outside the band are not touched;
//   * four table reads a pixel.
// z, winner words, the shadow buffer and every flag but the one lowered are left alone.  No atomics, no inline
// assembly, no scratch; LDS is dynamic only (its base stays 16-byte aligned).
constexpr int GRADE_THREADS = 256, GRADE_UNITS = TILE_W * TILE_H / 4 / GRADE_THREADS;  // units of a tile a lane owns
constexpr int GRADE_MAX_PER_CU = 8;  // workgroups of 256 lanes a CU holds by its waves

template <bool LDS, bool WORDS>
__global__ __launch_bounds__(GRADE_THREADS) void k_grade(GradeArgs a)
{
    static_assert(TILE_W == 128 && GRADE_UNITS == 2 && TILE_H == 16, "32 units to a row of a tile, two rounds of eight rows");
    extern __shared__ __align__(16) uint32_t s_lut[];
    const int32_t W = (int32_t)a.frame.width, H = (int32_t)a.frame.height;
    const uint32_t ntx = a.frame.ntx, n_tiles = a.frame.ntx * a.frame.nty, G = gridDim.x;
    const uint32_t n = a.rule.n, c0 = a.rule.c0;
    const bool in_place = a.out == a.fb;
    bool staged = !LDS;
    for (uint32_t k = blockIdx.x; k < n_tiles; k += G) {
        const uint32_t tyl = k / ntx, tx = (k % ntx + 5u * tyl + 13u * (tyl * ntx / G)) % ntx;
        const uint32_t t = tyl * ntx + tx;
        const bool clean = a.fbclean != nullptr && a.fbclean[t] != 0u;  // (workgroup-uniform)
        if (clean && in_place && c0 == 0u) continue;
        if (!clean && !staged) {  // (workgroup-uniform: the barrier is reached by all or none)
            const uint32_t pieces = (n * n * n + 3u) / 4u;  // (the device table is padded to whole pieces)
            for (uint32_t i = threadIdx.x; i < pieces; i += GRADE_THREADS)
                reinterpret_cast<uint4 *>(s_lut)[i] = reinterpret_cast<const uint4 *>(a.lut)[i];
            __syncthreads();
            staged = true;
        }
        const int32_t x = (int32_t)tx * TILE_W + 4 * (int32_t)(threadIdx.x % 32u);
        const int32_t y_first = (a.frame.ty_base + (int32_t)tyl) * TILE_H + (int32_t)(threadIdx.x / 32u);
        const int32_t n_px = min(4, W - x);  // (WORDS: 4, or the unit is outside)
        bool inside[GRADE_UNITS];
        size_t ci[GRADE_UNITS];
        uint32_t px[GRADE_UNITS][4];
#pragma unroll
        for (int h = 0; h < GRADE_UNITS; h++) {
            const int32_t y = y_first + 8 * h;
            inside[h] = x < W && y >= a.frame.band_y0 && y < a.frame.band_y1;
            ci[h] = inside[h] ? ((size_t)(H - 1 - y) * (size_t)W + (size_t)x) * 3u : 0u;
#pragma unroll
            for (int i = 0; i < 4; i++) px[h][i] = c0;
        }
        if (!clean) {
            // both units' loads first, then the arithmetic
#pragma unroll
            for (int h = 0; h < GRADE_UNITS; h++) {
                if (!inside[h]) continue;
                const uint8_t *q = a.fb + ci[h];
                if (WORDS) {
                    const uint32_t *qw = reinterpret_cast<const uint32_t *>(q);
                    const uint32_t w0 = qw[0], w1 = qw[1], w2 = qw[2];
                    px[h][0] = w0 & 0xFFFFFFu;
                    px[h][1] = (w0 >> 24) | ((w1 & 0xFFFFu) << 8);
                    px[h][2] = (w1 >> 16) | ((w2 & 0xFFu) << 16);
                    px[h][3] = w2 >> 8;
                } else {
#pragma unroll
                    for (int i = 0; i < 4; i++)
                        if (i < n_px) px[h][i] = grade_pack(q[3 * i], q[3 * i + 1], q[3 * i + 2]);
                }
            }
#pragma unroll
            for (int h = 0; h < GRADE_UNITS; h++) {
                if (!inside[h]) continue;
#pragma unroll
                for (int i = 0; i < 4; i++)
                    if (WORDS || i < n_px) px[h][i] = LDS ? grade_px(s_lut, n, px[h][i]) : grade_px(a.lut, n, px[h][i]);
            }
        }
#pragma unroll
        for (int h = 0; h < GRADE_UNITS; h++) {
            if (!inside[h]) continue;
            uint8_t *o = a.out + ci[h];
            if (WORDS) {
                uint32_t *ow = reinterpret_cast<uint32_t *>(o);
                ow[0] = px[h][0] | (px[h][1] << 24);
                ow[1] = (px[h][1] >> 8) | (px[h][2] << 16);
                ow[2] = (px[h][2] >> 16) | (px[h][3] << 8);
            } else {
#pragma unroll
                for (int i = 0; i < 4; i++)
                    if (i < n_px) {
                        o[3 * i + 0] = (uint8_t)(px[h][i] & 0xFFu);
                        o[3 * i + 1] = (uint8_t)((px[h][i] >> 8) & 0xFFu);
                        o[3 * i + 2] = (uint8_t)((px[h][i] >> 16) & 0xFFu);
                    }
            }
        }
        if (clean && a.lower_clean != nullptr) {  // (workgroup-uniform) the tile holds c0 != 0 now
            __syncthreads();
            if (threadIdx.x == 0u) a.lower_clean[t] = 0u;
        }
    }
}

// Layers (tr_scene_layer, tr_scene_layer_from_scene): a second image blended into the frame, into `out`, which may BE the
// frame (a pixel depends on itself and on the layer alone); tr_layer.h has the rule.  One workgroup of 256 lanes per
// 128 x 16 tile, over the tiles the clipped rectangle touches -- out of place over every tile: the rest is copied.
//   * units as in k_grade: four pixels of a row, twelve bytes, two units a lane eight rows apart.  WORDS: width % 4 == 0
//     and fb and out 4-byte aligned (z 16-byte with a WHERE flag; the launcher checks): a unit is three aligned words;
//     otherwise guarded bytes.  A unit the rectangle only partly covers blends its covered pixels and keeps the others;
//   * the layer's bytes for a unit start at any byte: the aligned words that cover the unit's COVERED bytes are loaded
//     and funnel-shifted into pixels (layer_fetch: four words for rgb8, five for an unaligned rgba8); a word that does
//     not overlap them is never loaded, the block's first and last word are put together from bytes where they reach
//     outside it.  FORMAT 2 is another scene's rgb8 frame behind its colour flags: a unit lies in one source tile row
//     and at most two source tile columns, and its pixels behind a raised flag are zeros without a load;
//   * the tile's own colour flag is workgroup-uniform (one scalar word): raised, d = 0 without a load.  In place a tile
//     the rectangle misses is not touched; a flagged tile under MULTIPLY or DARKEN stays black behind its flag; any other
//     flagged tile is stored whole (zeros and the blend) and lane 0 lowers the flag behind a barrier; an unflagged tile
//     loads and stores only the units the rectangle covers;
//   * WHERE: the tile's z flag is workgroup-uniform too.  Raised, nothing is drawn in the tile: WHERE_DRAWN takes the
//     tile as missed, WHERE_UNDRAWN covers it without reading z; otherwise z is read per covered unit (z is indexed y
//     up, the frame's rows top down).  It is the z flag that says "not drawn", never the colour flag;
//   * the mode is workgroup-uniform: one scalar switch a unit around the arithmetic of its four pixels.
// z, winner words, the shadow buffer and every flag but the one lowered are left alone.  No LDS, no atomics, no inline
// assembly, no scratch.
constexpr int LAYER_THREADS = 256, LAYER_UNITS = TILE_W * TILE_H / 4 / LAYER_THREADS;
constexpr int LAYER_FROM_SCENE = 2;  // (FORMAT beside LAYER_RGB8 and LAYER_RGBA8)

template <uint32_t MODE>
__device__ __forceinline__ void layer_unit(uint32_t d[4], const uint32_t s[4], const uint32_t cov[4], uint32_t m)
{
#pragma unroll
    for (int i = 0; i < 4; i++)
        if ((m >> i) & 1u) d[i] = layer_px<MODE>(s[i], d[i], cov[i]);
}

template <bool WORDS, int FORMAT, bool WHERE>
__global__ __launch_bounds__(LAYER_THREADS) void k_layer(LayerArgs a)
{
    static_assert(TILE_W == 128 && LAYER_UNITS == 2 && TILE_H == 16, "32 units to a row of a tile, two rounds of eight rows");
    constexpr int BPP = FORMAT == (int)LAYER_RGBA8 ? 4 : 3;
    const int32_t W = (int32_t)a.frame.width, H = (int32_t)a.frame.height;
    const uint32_t tx = a.gx0 + blockIdx.x % a.gnx, ty = a.gy0 + blockIdx.x / a.gnx, t = ty * a.frame.ntx + tx;
    const bool in_place = a.out == a.fb;
    const bool clean = a.fbclean != nullptr && a.fbclean[t] != 0u;  // (workgroup-uniform)
    const uint32_t mode = a.rule.mode;
    // does the clipped rectangle touch the tile?  (tile rows counted up, the rectangle's from the top)
    const int32_t tx0 = (int32_t)tx * TILE_W, tx1 = min(W, tx0 + TILE_W), yu0 = (int32_t)ty * TILE_H, yu1 = min(H, yu0 + TILE_H);
    bool hit = a.cx0 < tx1 && tx0 < a.cx1 && a.cr0 < H - yu0 && H - yu1 < a.cr1 && a.rule.opacity != 0u;
    bool read_z = false;
    if (WHERE) {
        const bool z_clean = a.zclean[t] != 0u;  // (workgroup-uniform) nothing is drawn in the tile
        if (z_clean && (a.rule.flags & LAYER_WHERE_DRAWN)) hit = false;
        read_z = hit && !z_clean;
    }
    if (in_place) {
        if (!hit) return;
        if (clean && (mode == LAYER_MULTIPLY || mode == LAYER_DARKEN)) return;  // black stays black behind its flag
    }
    const bool store_all = !in_place || clean;
    const int32_t x = tx0 + 4 * (int32_t)(threadIdx.x % 32u), row_first = yu0 + (int32_t)(threadIdx.x / 32u);
    const int32_t n_px = min(4, W - x);  // (WORDS: 4, or the unit is outside)
#pragma unroll
    for (int h = 0; h < LAYER_UNITS; h++) {
        const int32_t y = row_first + 8 * h, r = H - 1 - y;
        if (x >= W || y >= H) continue;
        // the unit's covered pixels: i0 .. i1 - 1
        int32_t i0 = 0, i1 = 0;
        if (hit && r >= a.cr0 && r < a.cr1) i0 = max(0, a.cx0 - x), i1 = min(n_px, a.cx1 - x);
        uint32_t m = i0 < i1 ? ((1u << i1) - 1u) & ~((1u << i0) - 1u) : 0u;
        if (!store_all && m == 0u) continue;
        const size_t ci = ((size_t)r * (size_t)W + (size_t)x) * 3u;
        uint32_t d[4] = { 0u, 0u, 0u, 0u };
        if (!clean) {
            const uint8_t *q = a.fb + ci;
            if (WORDS) {
                const uint32_t *qw = reinterpret_cast<const uint32_t *>(q);
                const uint32_t w0 = qw[0], w1 = qw[1], w2 = qw[2];
                d[0] = w0 & 0xFFFFFFu;
                d[1] = (w0 >> 24) | ((w1 & 0xFFFFu) << 8);
                d[2] = (w1 >> 16) | ((w2 & 0xFFu) << 16);
                d[3] = w2 >> 8;
            } else {
#pragma unroll
                for (int i = 0; i < 4; i++)
                    if (i < n_px) d[i] = grade_pack(q[3 * i], q[3 * i + 1], q[3 * i + 2]);
            }
        }
        if (m != 0u) {
            // the layer's pixels under the unit: pixel i of the unit is column lc + i of layer row lr
            const int32_t lc = x - a.rule.x, lr = r - a.rule.y;
            int32_t j0 = i0, j1 = i1;  // the pixels to load: the covered ones not behind a source flag
            if (FORMAT == LAYER_FROM_SCENE) {
                if (a.src_all_clean != 0u) j1 = j0;
                else if (a.src_clean != nullptr) {
                    const uint32_t *row = a.src_clean + (size_t)(((int32_t)a.rule.height - 1 - lr) / TILE_H) * a.src_ntx;
                    const int32_t ta = (lc + i0) / TILE_W, tb = (lc + i1 - 1) / TILE_W, ib = tb * TILE_W - lc;  // pixel ib begins tile tb
                    const bool fa = row[ta] != 0u, fb = ta == tb ? fa : row[tb] != 0u;
                    if (fa) j0 = ta == tb ? i1 : ib;
                    if (fb) j1 = ta == tb ? j0 : (fa ? j0 : ib);
                }
            }
            uint32_t s[4] = { 0xFF000000u, 0xFF000000u, 0xFF000000u, 0xFF000000u };
            if (j0 < j1) {
                const int64_t u0 = (int64_t)lr * (int64_t)a.rule.stride + (int64_t)lc * BPP;
                layer_fetch<BPP>(a.image, a.total, u0, u0 + j0 * BPP, u0 + j1 * BPP, s);
            }
            if (FORMAT == LAYER_FROM_SCENE) {
#pragma unroll
                for (int i = 0; i < 4; i++)
                    if (i < j0 || i >= j1) s[i] = 0xFF000000u;
            }
            uint32_t drawn = 0u;  // bit i: pixel i of the unit is drawn
            if (WHERE && read_z) {
                const float *zq = a.z + (size_t)y * (size_t)W + (size_t)x;
                if (WORDS) {
                    const float4 v = *reinterpret_cast<const float4 *>(zq);
                    drawn = (layer_drawn(v.x) ? 1u : 0u) | (layer_drawn(v.y) ? 2u : 0u) | (layer_drawn(v.z) ? 4u : 0u) | (layer_drawn(v.w) ? 8u : 0u);
                } else {
#pragma unroll
                    for (int i = 0; i < 4; i++)
                        if (((m >> i) & 1u) && layer_drawn(zq[i])) drawn |= 1u << i;
                }
            }
            uint32_t cov[4];
#pragma unroll
            for (int i = 0; i < 4; i++) cov[i] = layer_coverage(a.rule, s[i], ((drawn >> i) & 1u) != 0u);
            switch (mode) {  // (scalar)
            case LAYER_ADD: layer_unit<LAYER_ADD>(d, s, cov, m); break;
            case LAYER_MULTIPLY: layer_unit<LAYER_MULTIPLY>(d, s, cov, m); break;
            case LAYER_SCREEN: layer_unit<LAYER_SCREEN>(d, s, cov, m); break;
            case LAYER_LIGHTEN: layer_unit<LAYER_LIGHTEN>(d, s, cov, m); break;
            case LAYER_DARKEN: layer_unit<LAYER_DARKEN>(d, s, cov, m); break;
            case LAYER_DIFFERENCE: layer_unit<LAYER_DIFFERENCE>(d, s, cov, m); break;
            default: layer_unit<LAYER_NORMAL>(d, s, cov, m); break;
            }
        }
        uint8_t *o = a.out + ci;
        if (WORDS) {
            uint32_t *ow = reinterpret_cast<uint32_t *>(o);
            ow[0] = d[0] | (d[1] << 24);
            ow[1] = (d[1] >> 8) | (d[2] << 16);
            ow[2] = (d[2] >> 16) | (d[3] << 8);
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++)
                if (i < n_px) {
                    o[3 * i + 0] = (uint8_t)(d[i] & 0xFFu);
                    o[3 * i + 1] = (uint8_t)((d[i] >> 8) & 0xFFu);
                    o[3 * i + 2] = (uint8_t)((d[i] >> 16) & 0xFFu);
                }
        }
    }
    if (in_place && clean && a.lower != nullptr) {  // (workgroup-uniform) the tile holds the blend over zeros now
        __syncthreads();
        if (threadIdx.x == 0u) a.lower[t] = 0u;
    }
}

// Depth ramp (tr_scene_ramp): every pixel of the frame blended with the entry of the scene's 1-D rgba table that its own
// depth chooses, into `out`, which may BE the frame (a pixel depends on itself alone); tr_ramp.h has the rule.  k_grade's
// form: PERSISTENT workgroups -- as many as the machine holds at once, never more than there are tiles -- that stage the
// table (at most 4 KB) into LDS once and walk the 128 x 16 tiles of the frame under k_grade's permutation of a row's
// columns.  Staging per tile would add up to 4 KB to the 14 KB of colour and depth a tile moves.
//   * a unit is four pixels of a row: twelve bytes of colour and sixteen of depth; a lane takes two units of a tile, eight
//     rows apart.  WORDS: width % 4 == 0, fb and out 4-byte and z 16-byte aligned (the launcher checks): three aligned
//     words and one float4; otherwise guarded bytes and scalar z loads.  z is indexed y up, the frame's rows top down;
//   * the tile's z flag is workgroup-uniform (one scalar word).  Raised, nothing is drawn in the tile: no z is loaded,
//     the table is not needed (a workgroup whose tiles are all empty never stages it) and every pixel takes `undrawn`.
//     Where undrawn's coverage is 0 the tile is unchanged: in place it is not touched, out of place it is copied.  It is
//     the z flag that says "not drawn", never the colour flag;
//   * the tile's colour flag is workgroup-uniform too: raised, d = 0 without a load.  In place such a tile stays black
//     behind its flag under MULTIPLY and DARKEN; under any other mode it is stored whole and lane 0 lowers the flag
//     behind a barrier (every wave has read it by then) -- k_layer's rule;
//   * the mode and REPEAT are workgroup-uniform: one scalar switch a unit around the arithmetic of its four pixels, and a
//     `%` only under REPEAT.  A pixel that is not drawn computes a position like any other (the cast saturates, the clamp
//     keeps the index inside the table) and then takes `undrawn`: no divergence.
// z, winner words, the shadow buffer and every flag but the one lowered are left alone.  No atomics, no scratch; LDS is
// dynamic only (its base stays 16-byte aligned).
constexpr int RAMP_THREADS = 256, RAMP_UNITS = TILE_W * TILE_H / 4 / RAMP_THREADS;
constexpr int RAMP_MAX_PER_CU = 8;  // workgroups of 256 lanes a CU holds by its waves (8 x 4 KB of LDS at most)

template <uint32_t MODE>
__device__ __forceinline__ void ramp_unit(uint32_t d[4], const uint32_t e[4], uint32_t opacity, int32_t n_px)
{
#pragma unroll
    for (int i = 0; i < 4; i++)
        if (i < n_px) d[i] = layer_px<MODE>(e[i], d[i], ramp_coverage(e[i], opacity));
}

template <bool WORDS>
__global__ __launch_bounds__(RAMP_THREADS) void k_ramp(RampArgs a)
{
    static_assert(TILE_W == 128 && RAMP_UNITS == 2 && TILE_H == 16, "32 units to a row of a tile, two rounds of eight rows");
    extern __shared__ __align__(16) uint32_t s_ramp[];
    const int32_t W = (int32_t)a.frame.width, H = (int32_t)a.frame.height;
    const uint32_t ntx = a.frame.ntx, n_tiles = a.frame.ntx * a.frame.nty, G = gridDim.x;
    const RampRule q = a.rule;
    const bool in_place = a.out == a.fb;
    const uint32_t und_cov = ramp_coverage(q.undrawn, q.opacity);
    const bool keeps_black = q.mode == LAYER_MULTIPLY || q.mode == LAYER_DARKEN;
    bool staged = false;
    for (uint32_t k = blockIdx.x; k < n_tiles; k += G) {
        const uint32_t ty = k / ntx, tx = (k % ntx + 5u * ty + 13u * (ty * ntx / G)) % ntx;
        const uint32_t t = ty * ntx + tx;
        const bool clean = a.fbclean != nullptr && a.fbclean[t] != 0u;  // (workgroup-uniform)
        const bool empty = a.zclean[t] != 0u;                           // (workgroup-uniform) nothing is drawn in the tile
        const bool blend = !empty || und_cov != 0u;
        if (in_place && (!blend || (clean && keeps_black))) continue;
        if (!empty && !staged) {  // (workgroup-uniform: the barrier is reached by all or none)
            const uint32_t pieces = (q.n + 3u) / 4u;  // (the device table is padded to whole pieces)
            for (uint32_t i = threadIdx.x; i < pieces; i += RAMP_THREADS)
                reinterpret_cast<uint4 *>(s_ramp)[i] = reinterpret_cast<const uint4 *>(a.table)[i];
            __syncthreads();
            staged = true;
        }
        const int32_t x = (int32_t)tx * TILE_W + 4 * (int32_t)(threadIdx.x % 32u);
        const int32_t y_first = (int32_t)ty * TILE_H + (int32_t)(threadIdx.x / 32u);
        const int32_t n_px = WORDS ? 4 : min(4, W - x);  // (WORDS: 4, or the unit is outside)
        bool inside[RAMP_UNITS];
        size_t ci[RAMP_UNITS];
        uint32_t d[RAMP_UNITS][4];
        float zv[RAMP_UNITS][4];
        // both units' loads first, then the arithmetic
#pragma unroll
        for (int h = 0; h < RAMP_UNITS; h++) {
            const int32_t y = y_first + 8 * h;
            inside[h] = x < W && y < H;
            ci[h] = inside[h] ? ((size_t)(H - 1 - y) * (size_t)W + (size_t)x) * 3u : 0u;
#pragma unroll
            for (int i = 0; i < 4; i++) d[h][i] = 0u, zv[h][i] = 0.0f;
            if (!inside[h]) continue;
            if (!clean) {
                const uint8_t *c = a.fb + ci[h];
                if (WORDS) {
                    const uint32_t *cw = reinterpret_cast<const uint32_t *>(c);
                    const uint32_t w0 = cw[0], w1 = cw[1], w2 = cw[2];
                    d[h][0] = w0 & 0xFFFFFFu;
                    d[h][1] = (w0 >> 24) | ((w1 & 0xFFFFu) << 8);
                    d[h][2] = (w1 >> 16) | ((w2 & 0xFFu) << 16);
                    d[h][3] = w2 >> 8;
                } else {
#pragma unroll
                    for (int i = 0; i < 4; i++)
                        if (i < n_px) d[h][i] = grade_pack(c[3 * i], c[3 * i + 1], c[3 * i + 2]);
                }
            }
            if (!empty) {
                const float *zq = a.z + (size_t)y * (size_t)W + (size_t)x;
                if (WORDS) {
                    const float4 v = *reinterpret_cast<const float4 *>(zq);
                    zv[h][0] = v.x, zv[h][1] = v.y, zv[h][2] = v.z, zv[h][3] = v.w;
                } else {
#pragma unroll
                    for (int i = 0; i < 4; i++)
                        if (i < n_px) zv[h][i] = zq[i];
                }
            }
        }
        if (blend) {
#pragma unroll
            for (int h = 0; h < RAMP_UNITS; h++) {
                if (!inside[h]) continue;
                uint32_t e[4];
#pragma unroll
                for (int i = 0; i < 4; i++) e[i] = empty ? q.undrawn : ramp_source(s_ramp, zv[h][i], q);
                switch (q.mode) {  // (scalar)
                case LAYER_ADD: ramp_unit<LAYER_ADD>(d[h], e, q.opacity, n_px); break;
                case LAYER_MULTIPLY: ramp_unit<LAYER_MULTIPLY>(d[h], e, q.opacity, n_px); break;
                case LAYER_SCREEN: ramp_unit<LAYER_SCREEN>(d[h], e, q.opacity, n_px); break;
                case LAYER_LIGHTEN: ramp_unit<LAYER_LIGHTEN>(d[h], e, q.opacity, n_px); break;
                case LAYER_DARKEN: ramp_unit<LAYER_DARKEN>(d[h], e, q.opacity, n_px); break;
                case LAYER_DIFFERENCE: ramp_unit<LAYER_DIFFERENCE>(d[h], e, q.opacity, n_px); break;
                default: ramp_unit<LAYER_NORMAL>(d[h], e, q.opacity, n_px); break;
                }
            }
        }
#pragma unroll
        for (int h = 0; h < RAMP_UNITS; h++) {
            if (!inside[h]) continue;
            uint8_t *o = a.out + ci[h];
            if (WORDS) {
                uint32_t *ow = reinterpret_cast<uint32_t *>(o);
                ow[0] = d[h][0] | (d[h][1] << 24);
                ow[1] = (d[h][1] >> 8) | (d[h][2] << 16);
                ow[2] = (d[h][2] >> 16) | (d[h][3] << 8);
            } else {
#pragma unroll
                for (int i = 0; i < 4; i++)
                    if (i < n_px) {
                        o[3 * i + 0] = (uint8_t)(d[h][i] & 0xFFu);
                        o[3 * i + 1] = (uint8_t)((d[h][i] >> 8) & 0xFFu);
                        o[3 * i + 2] = (uint8_t)((d[h][i] >> 16) & 0xFFu);
                    }
            }
        }
        if (in_place && clean && a.lower != nullptr) {  // (workgroup-uniform) the tile holds the blend over zeros now
            __syncthreads();
            if (threadIdx.x == 0u) a.lower[t] = 0u;
        }
    }
}

// Lines (tr_scene_lines): the scene's table of segments drawn into the frame, depth-tested against the frame's own z,
// into `out`, which may BE the frame (a pixel depends on itself and the table alone); tr_lines.h has the rule.  The first
// kernel here that SCATTERS: a segment's steps land on pixels, and a pixel's winner is a maximum over what lands on it.
// One workgroup of 256 lanes per 128 x 16 tile: in place over the non-empty tiles alone (a.tiles, the host knows them: the
// grid is exact), out of place over every tile -- the rest is copied, as k_layer does.
//   * a tile with a list clears 2048 u64 words in LDS (16 KB) and, under TEST, stages its z (8 KB; f32::MIN without a
//     load behind a raised z flag or outside the frame), then walks its list: WAVES take segments (the list index and so
//     the segment's 32 bytes are wave-uniform), LANES take steps k, clipped first to the tile's range along the segment's
//     major axis, so the part of a long segment outside the tile costs nothing; a step loops over the width's minor
//     offsets, and every candidate inside the tile that survives the test offers its word by an LDS atomicMax.  A maximum
//     does not care in which order the lanes arrive: the device equals the host in every byte;
//   * behind a barrier a pixel with a non-zero word fetches its winner's colour and blends (layer_px<NORMAL>); units as
//     in k_layer: four pixels of a row, two units a lane, WORDS: three aligned words, otherwise guarded bytes;
//   * in place an unflagged tile stores only the units with a winner; a tile behind a raised colour flag counts as zeros
//     and, iff it has a pixel with a winner (one __syncthreads_or), is stored whole and lane 0 lowers the flag behind a
//     barrier -- otherwise it is not touched.
// z, winner words, the shadow buffer and every flag but the one lowered are left alone.  No inline assembly, no scratch.
constexpr int LINES_THREADS = 256, LINES_WAVES = LINES_THREADS / 64, LINES_UNITS = TILE_W * TILE_H / 4 / LINES_THREADS;

template <bool WORDS, bool TEST>
__global__ __launch_bounds__(LINES_THREADS) void k_lines(LinesArgs a)
{
    static_assert(TILE_W == 128 && LINES_UNITS == 2 && TILE_H == 16, "32 units to a row of a tile, two rounds of eight rows");
    __shared__ unsigned long long s_word[TILE_W * TILE_H];
    __shared__ float s_z[TEST ? TILE_W * TILE_H : 1];
    const int32_t W = (int32_t)a.frame.width, H = (int32_t)a.frame.height;
    const uint32_t t = a.tiles != nullptr ? a.tiles[blockIdx.x] : blockIdx.x;  // (workgroup-uniform)
    const uint32_t tx = t % a.frame.ntx, ty = t / a.frame.ntx;
    const bool in_place = a.out == a.fb;
    const bool clean = a.fbclean != nullptr && a.fbclean[t] != 0u;  // (workgroup-uniform)
    const uint32_t e0 = a.offsets[t], e1 = a.offsets[t + 1u];
    const bool listed = e1 > e0 && a.rule.opacity != 0u;            // (workgroup-uniform)
    const int32_t tx0 = (int32_t)tx * TILE_W, ty0 = (int32_t)ty * TILE_H;
    const int32_t tw = min(TILE_W, W - tx0), th = min(TILE_H, H - ty0);  // the tile inside the frame
    if (listed) {
        const bool z_clean = TEST && a.zclean[t] != 0u;  // (workgroup-uniform) nothing is drawn in the tile
        for (int32_t i = (int32_t)threadIdx.x; i < TILE_W * TILE_H; i += LINES_THREADS) {
            s_word[i] = 0ull;
            if (TEST) {
                const int32_t lx = i % TILE_W, ly = i / TILE_W;
                float v = bits_f32(TR_F32_MIN_BITS);
                if (!z_clean && lx < tw && ly < th) v = a.z[(size_t)(ty0 + ly) * (size_t)W + (size_t)(tx0 + lx)];
                s_z[i] = v;
            }
        }
        __syncthreads();
        const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / 64u));
        const int32_t lane = (int32_t)(threadIdx.x % 64u);
        const int32_t o_lo = -(((int32_t)a.rule.width - 1) / 2), o_hi = (int32_t)a.rule.width / 2;
        for (uint32_t e = e0 + wave; e < e1; e += (uint32_t)LINES_WAVES) {
            const uint32_t index = a.entries[e];
            const LineGeom g = lines_geom(a.lines[index]);
            const Recip rn = lines_recip(g);
            int32_t ks, ke;  // the steps inside the tile's range along the major axis
            if (g.xmajor) lines_steps(g, tx0, tx0 + tw - 1, &ks, &ke);
            else lines_steps(g, ty0, ty0 + th - 1, &ks, &ke);
            for (int32_t k = ks + lane; k <= ke; k += 64) {
                const int32_t bc = lines_minor(g, k);
                const float zl = lines_depth(g, k, rn, a.rule.bias);
                const unsigned long long word = lines_word(zl, index, a.rule.flags);
                for (int32_t o = o_lo; o <= o_hi; o++) {
                    const int32_t lx = (g.xmajor ? g.a0 + k : bc + o) - tx0, ly = (g.xmajor ? bc + o : g.a0 + k) - ty0;
                    if (lx < 0 || lx >= tw || ly < 0 || ly >= th) continue;
                    const int32_t p = ly * TILE_W + lx;  // (0 .. 2047: inside both arrays)
                    if (TEST && !lines_survives(zl, s_z[p])) continue;
                    atomicMax(&s_word[p], word);
                }
            }
        }
        __syncthreads();
    }
    const int32_t x = tx0 + 4 * (int32_t)(threadIdx.x % 32u), row_first = ty0 + (int32_t)(threadIdx.x / 32u);
    const int32_t n_px = min(4, W - x);  // (WORDS: 4, or the unit is outside)
    uint32_t win[LINES_UNITS][4];        // the winner's index + 1, or 0
    bool any = false;
#pragma unroll
    for (int h = 0; h < LINES_UNITS; h++) {
        const int32_t y = row_first + 8 * h;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            win[h][i] = 0u;
            if (listed && y < H && i < n_px) win[h][i] = (uint32_t)s_word[(y - ty0) * TILE_W + (x - tx0) + i];
            any = any || win[h][i] != 0u;
        }
    }
    if (in_place) {
        if (!listed) return;
        if (clean && __syncthreads_or(any ? 1 : 0) == 0) return;  // (workgroup-uniform) no winner: the flag stays up
    }
    const bool store_all = !in_place || clean;
#pragma unroll
    for (int h = 0; h < LINES_UNITS; h++) {
        const int32_t y = row_first + 8 * h, r = H - 1 - y;
        if (x >= W || y >= H) continue;
        const bool unit_any = (win[h][0] | win[h][1] | win[h][2] | win[h][3]) != 0u;
        if (!store_all && !unit_any) continue;
        const size_t ci = ((size_t)r * (size_t)W + (size_t)x) * 3u;
        uint32_t d[4] = { 0u, 0u, 0u, 0u };
        if (!clean) {
            const uint8_t *q = a.fb + ci;
            if (WORDS) {
                const uint32_t *qw = reinterpret_cast<const uint32_t *>(q);
                const uint32_t w0 = qw[0], w1 = qw[1], w2 = qw[2];
                d[0] = w0 & 0xFFFFFFu;
                d[1] = (w0 >> 24) | ((w1 & 0xFFFFu) << 8);
                d[2] = (w1 >> 16) | ((w2 & 0xFFu) << 16);
                d[3] = w2 >> 8;
            } else {
#pragma unroll
                for (int i = 0; i < 4; i++)
                    if (i < n_px) d[i] = grade_pack(q[3 * i], q[3 * i + 1], q[3 * i + 2]);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; i++)
            if (win[h][i] != 0u) d[i] = lines_px(a.lines[win[h][i] - 1u].rgba, d[i], a.rule.opacity);
        uint8_t *o = a.out + ci;
        if (WORDS) {
            uint32_t *ow = reinterpret_cast<uint32_t *>(o);
            ow[0] = d[0] | (d[1] << 24);
            ow[1] = (d[1] >> 8) | (d[2] << 16);
            ow[2] = (d[2] >> 16) | (d[3] << 8);
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++)
                if (i < n_px) {
                    o[3 * i + 0] = (uint8_t)(d[i] & 0xFFu);
                    o[3 * i + 1] = (uint8_t)((d[i] >> 8) & 0xFFu);
                    o[3 * i + 2] = (uint8_t)((d[i] >> 16) & 0xFFu);
                }
        }
    }
    if (in_place && clean && a.lower != nullptr) {  // (workgroup-uniform) the tile holds the lines over zeros now
        __syncthreads();
        if (threadIdx.x == 0u) a.lower[t] = 0u;
    }
}

// Distance field (tr_scene_distance, tr_scene_distance_ramp): tr_distance.h has the rule and the three passes.  The
// three field kernels share one geometry: a WAVE is 64 consecutive pixels of one row -- one mask word --, a workgroup
// four such rows; the grid is (words a row, rows / 4).  Rows are counted top down, like the frame buffer's.
//   k_dist_mask : a lane's pixel is a seed or not; one ballot is the word and lane 0 stores it.  The wave lies in one
//                 128 x 16 tile: behind a raised z flag (DRAWN) nothing is drawn, behind a raised colour flag (KEY) the
//                 pixels are black -- constant words without a load.  Bits past the width are 0, also under INVERT.
//   k_dist_row  : a lane's row distance from the row's words (dist_row_exact: at most nine words, no scan), stored as
//                 a byte; the wave's least summary byte (five shuffles) goes to summary[row][word].
//   k_dist      : the column search of dist_column, its bytes read from memory (a wave's tap is 64 consecutive bytes;
//                 neighbouring rows' waves read the same lines from L2).  Before it, the wave reads the summary bytes of
//                 its word's column over the 2 R + 1 rows in reach, at most eight a lane: where none is in reach no tap can
//                 give a value <= R^2 and the wave stores DIST_FAR without a search.
// No LDS, no atomics, no scratch; every index is guarded by the width and the height.
constexpr int DIST_THREADS = 256, DIST_ROWS = DIST_THREADS / 64;

template <bool KEY>
__global__ __launch_bounds__(DIST_THREADS) void k_dist_mask(DistArgs a)
{
    const uint32_t W = a.frame.width, H = a.frame.height, wpr = dist_words_per_row(W);
    const uint32_t seg = blockIdx.x, r = blockIdx.y * DIST_ROWS + threadIdx.x / 64u, lane = threadIdx.x % 64u;
    if (seg >= wpr || r >= H) return;  // (wave-uniform)
    const uint32_t x = seg * 64u + lane, y = H - 1u - r;
    const uint32_t t = (y / TILE_H) * a.frame.ntx + (seg * 64u) / TILE_W;
    const bool flagged = KEY ? (a.fbclean != nullptr && a.fbclean[t] != 0u) : a.zclean[t] != 0u;  // (wave-uniform)
    bool seed = false;
    if (flagged) {
        seed = KEY ? dist_seed_key(0u, a.rule.threshold) : false;
    } else if (x < W) {
        if (KEY) {
            const uint8_t *c = a.fb + ((size_t)r * W + x) * 3u;
            seed = dist_seed_key(grade_pack(c[0], c[1], c[2]), a.rule.threshold);
        } else {
            seed = dist_seed_drawn(a.z[(size_t)y * W + x]);
        }
    }
    seed = x < W && (seed != ((a.rule.flags & DIST_INVERT) != 0u));
    const unsigned long long word = __ballot(seed ? 1 : 0);
    if (lane == 0u) a.mask[(size_t)r * wpr + seg] = word;
}

__global__ __launch_bounds__(DIST_THREADS) void k_dist_row(DistArgs a)
{
    const uint32_t W = a.frame.width, H = a.frame.height, wpr = dist_words_per_row(W);
    const uint32_t seg = blockIdx.x, r = blockIdx.y * DIST_ROWS + threadIdx.x / 64u, lane = threadIdx.x % 64u;
    if (seg >= wpr || r >= H) return;  // (wave-uniform)
    const uint32_t x = seg * 64u + lane;
    uint32_t d = DIST_NONE;
    if (x < W) {
        d = dist_row_exact(a.mask + (size_t)r * wpr, wpr, x);
        a.h[(size_t)r * W + x] = (uint8_t)dist_row_byte(d);
    }
    uint32_t least = dist_summary_byte(d);
    for (int off = 32; off > 0; off >>= 1) least = min(least, (uint32_t)__shfl_xor((int)least, off, 64));
    if (lane == 0u) a.summary[(size_t)r * wpr + seg] = (uint8_t)least;
}

__global__ __launch_bounds__(DIST_THREADS) void k_dist(DistArgs a)
{
    const uint32_t W = a.frame.width, H = a.frame.height, wpr = dist_words_per_row(W);
    const uint32_t seg = blockIdx.x, r = blockIdx.y * DIST_ROWS + threadIdx.x / 64u, lane = threadIdx.x % 64u;
    if (seg >= wpr || r >= H) return;  // (wave-uniform)
    const uint32_t x = seg * 64u + lane, R = a.rule.radius;
    bool reach = false;
    for (int32_t rr = (int32_t)r - (int32_t)R + (int32_t)lane; rr <= (int32_t)r + (int32_t)R; rr += 64)
        if (rr >= 0 && rr < (int32_t)H) reach = reach || dist_summary_reach(a.summary[(size_t)rr * wpr + seg], R);
    const bool search = __ballot(reach ? 1 : 0) != 0ull;  // (wave-uniform)
    if (x >= W) return;
    uint32_t d2 = DIST_FAR;
    if (search) {
        const uint32_t own = dist_own_row(a.h[(size_t)r * W + x], R, a.mask + (size_t)r * wpr, wpr, x);
        d2 = dist_column(a.h, W, x, r, H, R, own, nullptr);
    }
    a.field[(size_t)r * W + x] = (uint16_t)d2;
}

// The distance ramp's pointwise half (tr_scene_distance_ramp): every pixel of the frame blended with the table entry
// that its field value chooses, into `out`, which may BE the frame -- the field is complete before this kernel starts.
// k_ramp's form, with the u16 field in the place of the depth: persistent workgroups, the table staged in LDS once, a
// unit of four pixels (twelve bytes of colour, eight of field) and two units a lane; WORDS as there, the field 8-byte
// aligned.  A tile's pixels are all FAR or not by one __syncthreads_or over the loaded field: all FAR, the table is not
// needed and every pixel takes `far`; where far's coverage is 0 the tile is unchanged -- in place it is not touched, and
// a raised colour flag stays up.  A tile behind a raised colour flag counts as zeros; in place it stays black behind its
// flag under MULTIPLY and DARKEN, under any other mode it is stored whole and lane 0 lowers the flag behind a barrier.
template <bool WORDS>
__global__ __launch_bounds__(RAMP_THREADS) void k_dist_apply(DistApplyArgs a)
{
    extern __shared__ __align__(16) uint32_t s_ramp[];
    const int32_t W = (int32_t)a.frame.width, H = (int32_t)a.frame.height;
    const uint32_t ntx = a.frame.ntx, n_tiles = a.frame.ntx * a.frame.nty, G = gridDim.x;
    const DistRampRule q = a.rule;
    const bool in_place = a.out == a.fb;
    const uint32_t far_cov = ramp_coverage(q.far, q.opacity);
    const bool keeps_black = q.mode == LAYER_MULTIPLY || q.mode == LAYER_DARKEN;
    bool staged = false;
    for (uint32_t k = blockIdx.x; k < n_tiles; k += G) {
        const uint32_t ty = k / ntx, tx = (k % ntx + 5u * ty + 13u * (ty * ntx / G)) % ntx;
        const uint32_t t = ty * ntx + tx;
        const bool clean = a.fbclean != nullptr && a.fbclean[t] != 0u;  // (workgroup-uniform)
        if (in_place && clean && keeps_black) continue;
        const int32_t x = (int32_t)tx * TILE_W + 4 * (int32_t)(threadIdx.x % 32u);
        const int32_t y_first = (int32_t)ty * TILE_H + (int32_t)(threadIdx.x / 32u);
        const int32_t n_px = WORDS ? 4 : min(4, W - x);  // (WORDS: 4, or the unit is outside)
        bool inside[RAMP_UNITS];
        size_t pi[RAMP_UNITS];
        uint32_t d[RAMP_UNITS][4], f[RAMP_UNITS][4];
        bool mine = false;
#pragma unroll
        for (int h = 0; h < RAMP_UNITS; h++) {
            const int32_t y = y_first + 8 * h;
            inside[h] = x < W && y < H;
            pi[h] = inside[h] ? (size_t)(H - 1 - y) * (size_t)W + (size_t)x : 0u;
#pragma unroll
            for (int i = 0; i < 4; i++) d[h][i] = 0u, f[h][i] = DIST_FAR;
            if (!inside[h]) continue;
            const uint16_t *fq = a.field + pi[h];
            if (WORDS) {
                const uint2 v = *reinterpret_cast<const uint2 *>(fq);
                f[h][0] = v.x & 0xFFFFu, f[h][1] = v.x >> 16, f[h][2] = v.y & 0xFFFFu, f[h][3] = v.y >> 16;
            } else {
#pragma unroll
                for (int i = 0; i < 4; i++)
                    if (i < n_px) f[h][i] = fq[i];
            }
#pragma unroll
            for (int i = 0; i < 4; i++) mine = mine || f[h][i] != DIST_FAR;
        }
        const bool near = __syncthreads_or((int)mine) != 0;  // (workgroup-uniform) the tile has a pixel within reach
        const bool blend = near || far_cov != 0u;
        if (in_place && !blend) continue;
        if (near && !staged) {  // (workgroup-uniform: the barrier is reached by all or none)
            const uint32_t pieces = (q.n + 3u) / 4u;  // (the device table is padded to whole pieces)
            for (uint32_t i = threadIdx.x; i < pieces; i += RAMP_THREADS)
                reinterpret_cast<uint4 *>(s_ramp)[i] = reinterpret_cast<const uint4 *>(a.table)[i];
            __syncthreads();
            staged = true;
        }
        if (!clean) {
#pragma unroll
            for (int h = 0; h < RAMP_UNITS; h++) {
                if (!inside[h]) continue;
                const uint8_t *c = a.fb + pi[h] * 3u;
                if (WORDS) {
                    const uint32_t *cw = reinterpret_cast<const uint32_t *>(c);
                    const uint32_t w0 = cw[0], w1 = cw[1], w2 = cw[2];
                    d[h][0] = w0 & 0xFFFFFFu;
                    d[h][1] = (w0 >> 24) | ((w1 & 0xFFFFu) << 8);
                    d[h][2] = (w1 >> 16) | ((w2 & 0xFFu) << 16);
                    d[h][3] = w2 >> 8;
                } else {
#pragma unroll
                    for (int i = 0; i < 4; i++)
                        if (i < n_px) d[h][i] = grade_pack(c[3 * i], c[3 * i + 1], c[3 * i + 2]);
                }
            }
        }
        if (blend) {
#pragma unroll
            for (int h = 0; h < RAMP_UNITS; h++) {
                if (!inside[h]) continue;
                uint32_t e[4], cov[4];
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    e[i] = near ? dist_source(s_ramp, f[h][i], q) : q.far;
                    cov[i] = dist_coverage(e[i], f[h][i], q);
                }
#pragma unroll
                for (int i = 0; i < 4; i++)
                    if (i < n_px) d[h][i] = layer_px_by(q.mode, e[i], d[h][i], cov[i]);  // (the mode is scalar)
            }
        }
#pragma unroll
        for (int h = 0; h < RAMP_UNITS; h++) {
            if (!inside[h]) continue;
            uint8_t *o = a.out + pi[h] * 3u;
            if (WORDS) {
                uint32_t *ow = reinterpret_cast<uint32_t *>(o);
                ow[0] = d[h][0] | (d[h][1] << 24);
                ow[1] = (d[h][1] >> 8) | (d[h][2] << 16);
                ow[2] = (d[h][2] >> 16) | (d[h][3] << 8);
            } else {
#pragma unroll
                for (int i = 0; i < 4; i++)
                    if (i < n_px) {
                        o[3 * i + 0] = (uint8_t)(d[h][i] & 0xFFu);
                        o[3 * i + 1] = (uint8_t)((d[h][i] >> 8) & 0xFFu);
                        o[3 * i + 2] = (uint8_t)((d[h][i] >> 16) & 0xFFu);
                    }
            }
        }
        if (in_place && clean && a.lower != nullptr) {  // (workgroup-uniform) the tile holds the blend over zeros now
            __syncthreads();
            if (threadIdx.x == 0u) a.lower[t] = 0u;
        }
    }
}

// Projector (tr_scene_projector): an image cast onto the frame's drawn pixels from a second camera, optionally shadowed
// by a second scene's depth, into `out`, which may BE the frame (a pixel depends on itself, the image and the occluder
// alone); tr_projector.h has the rule.  k_layer's form: one workgroup of 256 lanes per 128 x 16 tile of the frame, every
// tile launched (where the image lands is known only per pixel).
//   * units as in k_ramp: four pixels of a row, twelve bytes of colour and sixteen of depth, two units a lane eight rows
//     apart.  WORDS: width % 4 == 0, fb and out 4-byte and z 16-byte aligned (the launcher checks); otherwise guarded
//     bytes and scalar z loads.  z is indexed y up, the frame's rows top down;
//   * the tile's z flag is workgroup-uniform (one scalar word).  Raised, nothing is drawn in the tile and nothing is cast
//     on it: in place it is not touched and nothing of it is loaded, out of place it is copied (zeros behind a raised
//     colour flag).  It is the z flag that says "not drawn", never the colour flag;
//   * the tile's colour flag is workgroup-uniform too: raised, d = 0 without a load.  In place such a tile stays black
//     behind its flag under MULTIPLY and DARKEN; under any other mode the workgroup votes (__syncthreads_or) whether a
//     pixel of it is covered -- drawn and accepted by every step --: if so the tile is stored whole and lane 0 lowers the
//     flag (the vote is the barrier behind which every wave has read it), otherwise it is not touched.  An unflagged tile
//     in place stores only the units with a covered pixel;
//   * the image's texels and the occluder's depths are gathered straight from memory by the rule's own functions: byte
//     loads at any address and stride, float loads; a texel of weight 0 is never loaded, so no byte outside the image
//     and no float outside the occluder is.  An occluder texel behind a raised z flag of the OCCLUDER's tile grid counts
//     as f32::MIN without a load: its stale memory never decides a pixel;
//   * the reciprocal is IEEE's (recip_of, tr_math.h), no hardware approximation; the mode is workgroup-uniform: one
//     scalar switch a unit around the blend of its four pixels.
// z, winner words, the shadow buffer and every flag but the one lowered are left alone.  No atomics, no inline assembly,
// no scratch; the only LDS is the vote's own 256 bytes.
constexpr int PROJECTOR_THREADS = 256, PROJECTOR_UNITS = TILE_W * TILE_H / 4 / PROJECTOR_THREADS;

struct ProjectorDeviceZ {
    const float *z;
    const uint32_t *clean;
    uint32_t ntx, pw;
    __device__ __forceinline__ float operator()(int32_t i, int32_t j) const
    {
        if (clean[(uint32_t)j / (uint32_t)TILE_H * ntx + (uint32_t)i / (uint32_t)TILE_W] != 0u) return bits_f32(TR_F32_MIN_BITS);
        return z[(size_t)j * (size_t)pw + (size_t)i];
    }
};

template <bool WORDS>
__global__ __launch_bounds__(PROJECTOR_THREADS) void k_projector(ProjectorArgs a)
{
    static_assert(TILE_W == 128 && PROJECTOR_UNITS == 2 && TILE_H == 16, "32 units to a row of a tile, two rounds of eight rows");
    const int32_t W = (int32_t)a.frame.width, H = (int32_t)a.frame.height;
    const uint32_t t = blockIdx.x, tx = t % a.frame.ntx, ty = t / a.frame.ntx;
    const ProjectorRule &q = a.rule;
    const bool in_place = a.out == a.fb;
    const bool clean = a.fbclean != nullptr && a.fbclean[t] != 0u;  // (workgroup-uniform)
    const bool empty = a.zclean[t] != 0u;                           // (workgroup-uniform) nothing is drawn in the tile
    if (in_place && (empty || (clean && (q.mode == LAYER_MULTIPLY || q.mode == LAYER_DARKEN)))) return;
    const ProjectorDeviceZ zo = { a.occ_z, a.occ_zclean, a.occ_ntx, q.pw };
    const int32_t x = (int32_t)tx * TILE_W + 4 * (int32_t)(threadIdx.x % 32u);
    const int32_t y_first = (int32_t)ty * TILE_H + (int32_t)(threadIdx.x / 32u);
    const int32_t n_px = WORDS ? 4 : min(4, W - x);  // (WORDS: 4, or the unit is outside)
    bool inside[PROJECTOR_UNITS];
    size_t ci[PROJECTOR_UNITS];
    uint32_t d[PROJECTOR_UNITS][4], m[PROJECTOR_UNITS];
#pragma unroll
    for (int h = 0; h < PROJECTOR_UNITS; h++) {
        const int32_t y = y_first + 8 * h;
        inside[h] = x < W && y < H;
        ci[h] = inside[h] ? ((size_t)(H - 1 - y) * (size_t)W + (size_t)x) * 3u : 0u;
        m[h] = 0u;
#pragma unroll
        for (int i = 0; i < 4; i++) d[h][i] = 0u;
        if (!inside[h]) continue;
        if (!clean) {
            const uint8_t *c = a.fb + ci[h];
            if (WORDS) {
                const uint32_t *cw = reinterpret_cast<const uint32_t *>(c);
                const uint32_t w0 = cw[0], w1 = cw[1], w2 = cw[2];
                d[h][0] = w0 & 0xFFFFFFu;
                d[h][1] = (w0 >> 24) | ((w1 & 0xFFFFu) << 8);
                d[h][2] = (w1 >> 16) | ((w2 & 0xFFu) << 16);
                d[h][3] = w2 >> 8;
            } else {
#pragma unroll
                for (int i = 0; i < 4; i++)
                    if (i < n_px) d[h][i] = grade_pack(c[3 * i], c[3 * i + 1], c[3 * i + 2]);
            }
        }
        if (empty) continue;
        float zv[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
        const float *zq = a.z + (size_t)y * (size_t)W + (size_t)x;
        if (WORDS) {
            const float4 v = *reinterpret_cast<const float4 *>(zq);
            zv[0] = v.x, zv[1] = v.y, zv[2] = v.z, zv[3] = v.w;
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++)
                if (i < n_px) zv[i] = zq[i];
        }
        uint32_t s[4] = { 0u, 0u, 0u, 0u }, cov[4] = { 0u, 0u, 0u, 0u };
#pragma unroll
        for (int i = 0; i < 4; i++)
            if (i < n_px && projector_source(q, a.image, zo, x + i, y, zv[i], s[i], cov[i])) m[h] |= 1u << i;
        if (m[h] == 0u) continue;
        switch (q.mode) {  // (scalar)
        case LAYER_ADD: layer_unit<LAYER_ADD>(d[h], s, cov, m[h]); break;
        case LAYER_MULTIPLY: layer_unit<LAYER_MULTIPLY>(d[h], s, cov, m[h]); break;
        case LAYER_SCREEN: layer_unit<LAYER_SCREEN>(d[h], s, cov, m[h]); break;
        case LAYER_LIGHTEN: layer_unit<LAYER_LIGHTEN>(d[h], s, cov, m[h]); break;
        case LAYER_DARKEN: layer_unit<LAYER_DARKEN>(d[h], s, cov, m[h]); break;
        case LAYER_DIFFERENCE: layer_unit<LAYER_DIFFERENCE>(d[h], s, cov, m[h]); break;
        default: layer_unit<LAYER_NORMAL>(d[h], s, cov, m[h]); break;
        }
    }
    bool store_all = !in_place;
    if (in_place && clean) {  // (workgroup-uniform: the vote is reached by all or none)
        store_all = __syncthreads_or((int)(m[0] | m[1])) != 0;
        if (!store_all) return;
    }
#pragma unroll
    for (int h = 0; h < PROJECTOR_UNITS; h++) {
        if (!inside[h] || (!store_all && m[h] == 0u)) continue;
        uint8_t *o = a.out + ci[h];
        if (WORDS) {
            uint32_t *ow = reinterpret_cast<uint32_t *>(o);
            ow[0] = d[h][0] | (d[h][1] << 24);
            ow[1] = (d[h][1] >> 8) | (d[h][2] << 16);
            ow[2] = (d[h][2] >> 16) | (d[h][3] << 8);
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++)
                if (i < n_px) {
                    o[3 * i + 0] = (uint8_t)(d[h][i] & 0xFFu);
                    o[3 * i + 1] = (uint8_t)((d[h][i] >> 8) & 0xFFu);
                    o[3 * i + 2] = (uint8_t)((d[h][i] >> 16) & 0xFFu);
                }
        }
    }
    if (in_place && clean && a.lower != nullptr && threadIdx.x == 0u) a.lower[t] = 0u;  // the tile holds the blend over zeros now
}

// Relight (tr_scene_relight): coloured directional, point and spot lights laid on the frame's pixels from normals
// recovered out of its own z buffer, into `out`, which may BE the frame (a pixel's output depends on the depths around
// it and on its own colour alone); tr_relight.h has the rule.  k_outline's form: one workgroup of 256 lanes per 128 x 16
// tile of the frame, every tile launched.
//   * the tile's own z flag is workgroup-uniform.  Raised, nothing is drawn in the tile: in place it is not touched, no
//     load and no barrier; out of place it is copied (zeros behind a raised colour flag);
//   * staging: z of the tile and a halo of ONE pixel go to LDS as 18 rows of 136 floats that start 4 pixels left of the
//     tile (k_outline's rows: a 16-byte piece is aligned in memory and lies in one tile); a piece in a neighbour tile
//     whose z flag is up, or outside the frame, is filled with f32::MIN without a load.  The lane that stages a depth
//     computes its POSITION at once (relight_position: the matrix product and the one IEEE reciprocal) into three more
//     LDS planes, x = NaN where there is none -- once per staged pixel, where a pixel would otherwise pay for its own and
//     its four neighbours'.  Whether a staged pixel is inside the frame comes from its coordinates, never from LDS.
//     Only columns 3 .. 132 of a row are looked at.  39 KB of LDS; one barrier;
//   * a unit is four pixels of a row (k_grade's); a lane takes two units, eight rows apart.  A pixel with a position
//     reads its four neighbours' entries of every plane and runs the rule's own functions; the light table sits in the
//     kernel arguments and is read through scalar loads, the loop over it and every branch on a light's kind is
//     wave-uniform;
//   * colour: zeros behind a raised colour flag (no load), else the unit's twelve bytes.  Out of place every unit of the
//     tile is stored.  In place only units with a CHANGED pixel are stored; a flagged tile votes (__syncthreads_or)
//     whether one of its pixels changes: if so it is stored whole and lane 0 lowers the flag (the vote is the barrier
//     behind which every wave has read it), otherwise it is not touched.  Under MULTIPLY and DARKEN a flagged tile stays
//     black behind its flag and returns at once.
// WIDE: width % 4 == 0, z 16-byte and fb / out 4-byte aligned (the launcher checks): z in 16-byte pieces, a unit as three
// aligned words; otherwise the same through element accesses guarded by the width.  z, its flags, the winner words and
// the shadow buffer are only read.  No atomics, no scratch; no inline assembly beyond tr_math.h's conversions.
constexpr int RELIGHT_LDS_W = TILE_W + 8, RELIGHT_LDS_H = TILE_H + 2, RELIGHT_PLANE = RELIGHT_LDS_W * RELIGHT_LDS_H;
constexpr int RELIGHT_THREADS = 256, RELIGHT_UNITS = TILE_W * TILE_H / 4 / RELIGHT_THREADS;

// The tap at LDS index i of the four planes (z, then the position's x, y, z).
__device__ __forceinline__ RelightTap relight_tap(const float *s, int32_t i)
{
    RelightTap t;
    t.z = s[i];
    t.P = make3(s[RELIGHT_PLANE + i], s[2 * RELIGHT_PLANE + i], s[3 * RELIGHT_PLANE + i]);
    t.ok = t.P.x == t.P.x;
    return t;
}

template <bool WIDE>
__global__ __launch_bounds__(RELIGHT_THREADS) void k_relight(RelightArgs a)
{
    static_assert(TILE_W == 128 && TILE_H == 16 && RELIGHT_UNITS == 2, "32 units to a row of a tile, two rounds of eight rows");
    static_assert(RELIGHT_LDS_W % 4 == 0 && 4 * RELIGHT_PLANE * 4 <= 40 * 1024, "16-byte pieces; four planes in 40 KB");
    __shared__ __attribute__((aligned(16))) float s_t[4 * RELIGHT_PLANE];
    const uint32_t t = blockIdx.x;
    const int32_t W = (int32_t)a.frame.width, H = (int32_t)a.frame.height;
    const int32_t ntx = (int32_t)a.frame.ntx, nty = (int32_t)a.frame.nty;
    const int32_t tx = (int32_t)t % ntx, ty = (int32_t)t / ntx;
    const int32_t x0 = tx * TILE_W, y0 = ty * TILE_H;
    const RelightRule &q = a.rule;
    const bool in_place = a.out == a.fb;
    const bool clean = a.fbclean != nullptr && a.fbclean[t] != 0u;  // (workgroup-uniform)
    const bool empty = a.zclean[t] != 0u;                           // (workgroup-uniform) nothing is drawn in the tile
    if (in_place && (empty || (clean && (q.mode == LAYER_MULTIPLY || q.mode == LAYER_DARKEN)))) return;
    if (!empty) {  // (workgroup-uniform: the barrier is reached by all or none)
        // bit 3 * ay + ax: the tile at (tx + ax - 1, ty + ay - 1) reads as f32::MIN -- flag up, or no such tile
        uint32_t stale = 0u;
#pragma unroll
        for (int32_t ay = 0; ay < 3; ay++)
#pragma unroll
            for (int32_t ax = 0; ax < 3; ax++) {
                const int32_t nx = tx + ax - 1, ny = ty + ay - 1;
                bool up = nx < 0 || nx >= ntx || ny < 0 || ny >= nty;
                if (!up) up = a.zclean[ny * ntx + nx] != 0u;
                if (up) stale |= 1u << (3 * ay + ax);
            }
        // LDS row r is frame row y0 - 1 + r, LDS column c frame column x0 - 4 + c
        const float z_min = bits_f32(TR_F32_MIN_BITS), none = __builtin_nanf("");
        if (WIDE) {
            for (int32_t p = (int32_t)threadIdx.x; p < RELIGHT_LDS_H * (RELIGHT_LDS_W / 4); p += RELIGHT_THREADS) {
                const int32_t r = p / (RELIGHT_LDS_W / 4), j = p % (RELIGHT_LDS_W / 4);
                const int32_t px = x0 - 4 + 4 * j, py = y0 - 1 + r;
                const int32_t ax = j < 1 ? 0 : j < 1 + TILE_W / 4 ? 1 : 2, ay = py < y0 ? 0 : py < y0 + TILE_H ? 1 : 2;
                float zv[4] = { z_min, z_min, z_min, z_min };
                const bool live = ((stale >> (3 * ay + ax)) & 1u) == 0u && px < W && py < H;  // (WIDE: the piece is inside whole, or outside)
                if (live) {
                    const float4 v = *reinterpret_cast<const float4 *>(a.z + (size_t)py * (size_t)W + (size_t)px);
                    zv[0] = v.x, zv[1] = v.y, zv[2] = v.z, zv[3] = v.w;
                }
                float pv[3][4];
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const int32_t c = 4 * j + i;
                    vec3 P = make3(none, none, none);
                    if (live && c >= 3 && c <= 4 + TILE_W) {
                        vec3 got;
                        if (relight_position(q.u, px + i, py, zv[i], got)) P = got;
                    }
                    pv[0][i] = P.x, pv[1][i] = P.y, pv[2][i] = P.z;
                }
                const int32_t at = r * RELIGHT_LDS_W + 4 * j;
                *reinterpret_cast<float4 *>(&s_t[at]) = make_float4(zv[0], zv[1], zv[2], zv[3]);
#pragma unroll
                for (int k = 0; k < 3; k++)
                    *reinterpret_cast<float4 *>(&s_t[(k + 1) * RELIGHT_PLANE + at]) = make_float4(pv[k][0], pv[k][1], pv[k][2], pv[k][3]);
            }
        } else {
            for (int32_t p = (int32_t)threadIdx.x; p < RELIGHT_PLANE; p += RELIGHT_THREADS) {
                const int32_t r = p / RELIGHT_LDS_W, c = p % RELIGHT_LDS_W;
                if (c < 3 || c > 4 + TILE_W) continue;  // (no pixel of the tile looks at it)
                const int32_t px = x0 - 4 + c, py = y0 - 1 + r;
                const int32_t ax = c < 4 ? 0 : c < 4 + TILE_W ? 1 : 2, ay = py < y0 ? 0 : py < y0 + TILE_H ? 1 : 2;
                float v = z_min;
                vec3 P = make3(none, none, none);
                if (((stale >> (3 * ay + ax)) & 1u) == 0u && px < W && py < H) {
                    v = a.z[(size_t)py * (size_t)W + (size_t)px];
                    vec3 got;
                    if (relight_position(q.u, px, py, v, got)) P = got;
                }
                s_t[p] = v, s_t[RELIGHT_PLANE + p] = P.x, s_t[2 * RELIGHT_PLANE + p] = P.y, s_t[3 * RELIGHT_PLANE + p] = P.z;
            }
        }
        __syncthreads();
    }
    // the units of k_grade
    const int32_t ux = 4 * (int32_t)(threadIdx.x % 32u), x = x0 + ux, row_first = (int32_t)(threadIdx.x / 32u);
    const int32_t n_px = WIDE ? 4 : min(4, W - x);  // (WIDE: 4, or the unit is outside)
    bool inside[RELIGHT_UNITS];
    size_t ci[RELIGHT_UNITS];
    uint32_t d[RELIGHT_UNITS][4], m[RELIGHT_UNITS];  // m: bit i: pixel i of the unit has changed
#pragma unroll
    for (int h = 0; h < RELIGHT_UNITS; h++) {
        const int32_t row = row_first + 8 * h, y = y0 + row;
        inside[h] = x < W && y < H;
        ci[h] = inside[h] ? ((size_t)(H - 1 - y) * (size_t)W + (size_t)x) * 3u : 0u;
        m[h] = 0u;
#pragma unroll
        for (int i = 0; i < 4; i++) d[h][i] = 0u;
        if (!inside[h]) continue;
        if (!clean) {
            const uint8_t *c = a.fb + ci[h];
            if (WIDE) {
                const uint32_t *cw = reinterpret_cast<const uint32_t *>(c);
                const uint32_t w0 = cw[0], w1 = cw[1], w2 = cw[2];
                d[h][0] = w0 & 0xFFFFFFu;
                d[h][1] = (w0 >> 24) | ((w1 & 0xFFFFu) << 8);
                d[h][2] = (w1 >> 16) | ((w2 & 0xFFu) << 16);
                d[h][3] = w2 >> 8;
            } else {
#pragma unroll
                for (int i = 0; i < 4; i++)
                    if (i < n_px) d[h][i] = grade_pack(c[3 * i], c[3 * i + 1], c[3 * i + 2]);
            }
        }
        if (empty) continue;
        // the unit's window: LDS row row + 1, columns 3 + ux .. 8 + ux of it, 4 + ux .. 7 + ux of the rows around
        const int32_t mid = (row + 1) * RELIGHT_LDS_W + 4 + ux;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if (i >= n_px) continue;
            const RelightTap c = relight_tap(s_t, mid + i);
            if (!c.ok) continue;
            uint32_t v;
            if (relight_px(q, c, relight_tap(s_t, mid + i + 1), relight_tap(s_t, mid + i - 1), relight_tap(s_t, mid + i + RELIGHT_LDS_W),
                           relight_tap(s_t, mid + i - RELIGHT_LDS_W), d[h][i], v) &&
                v != d[h][i])
                d[h][i] = v, m[h] |= 1u << i;
        }
    }
    bool store_all = !in_place;
    if (in_place && clean) {  // (workgroup-uniform: the vote is reached by all or none)
        store_all = __syncthreads_or((int)(m[0] | m[1])) != 0;
        if (!store_all) return;
    }
#pragma unroll
    for (int h = 0; h < RELIGHT_UNITS; h++) {
        if (!inside[h] || (!store_all && m[h] == 0u)) continue;
        uint8_t *o = a.out + ci[h];
        if (WIDE) {
            uint32_t *ow = reinterpret_cast<uint32_t *>(o);
            ow[0] = d[h][0] | (d[h][1] << 24);
            ow[1] = (d[h][1] >> 8) | (d[h][2] << 16);
            ow[2] = (d[h][2] >> 16) | (d[h][3] << 8);
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++)
                if (i < n_px) {
                    o[3 * i + 0] = (uint8_t)(d[h][i] & 0xFFu);
                    o[3 * i + 1] = (uint8_t)((d[h][i] >> 8) & 0xFFu);
                    o[3 * i + 2] = (uint8_t)((d[h][i] >> 16) & 0xFFu);
                }
        }
    }
    if (in_place && clean && a.lower != nullptr && threadIdx.x == 0u) a.lower[t] = 0u;  // the tile holds the lights over zeros now
}

// Outlines (tr_scene_outline): ink laid over the frame's colour where its own z buffer has a silhouette, a depth step or
// a fold, into `out`, which may BE the frame (a pixel's output depends on the depths around it and on its own colour
// alone); tr_outline.h has the rule.  One workgroup of 256 lanes per 128 x 16 tile of the frame, the tiles of k_ao.
//   * the nine z flags of the 3 x 3 neighbourhood and the tile's own colour flag are workgroup-uniform (scalar loads; a
//     tile outside the grid counts as raised).  All nine raised: nothing is drawn within radius + 1 pixels, so the tile
//     has no ink -- no staging, no barrier, the colour phase below with empty masks;
//   * staging: z of the tile and a halo of radius + 1 pixels go to LDS as rows of 136 floats that start 4 pixels left of
//     the tile, so that a 16-byte piece is aligned in memory and lies in ONE tile: a piece in a tile whose z flag is up,
//     or outside the frame, is filled with f32::MIN without a load.  At most 24 rows: 13 KB.  "Outside the frame" is
//     not "not drawn": whether a neighbour EXISTS comes from the pixel's coordinates (outline_exist), never from LDS;
//   * seeds: for the tile and a halo of `radius` pixels, as bit rows -- a wave takes 64 consecutive pixels of a row,
//     every lane evaluates outline_kinds of its pixel from five LDS words, one ballot makes a 64-bit word, lane 0 stores
//     it.  At most 22 rows of three words;
//   * ink: a unit is four pixels of a row (k_grade's); a lane takes two units, eight rows apart.  It ORs the 2 r + 1 seed
//     rows around its row, shifted so that the unit's window of 4 + 2 r bits starts at bit 0 (one or two 64-bit words a
//     row, mostly the same words for a whole wave), and a pixel is inked when its 2 r + 1 bits of the window are not all
//     zero.  A vote (one barrier) says whether the tile has any ink;
//   * colour: base is paper under TR_OUTLINE_ONLY, zeros behind a raised colour flag (no load), else the unit's twelve
//     bytes.  Out of place every unit of the tile is stored.  In place without ONLY only units with ink are loaded and
//     stored, and a tile without ink is not touched -- but ink that reaches a FLAGGED tile stores the whole tile (zeros
//     and ink) and lane 0 lowers the flag behind a barrier: a flag that stays up still means "cleared colour, memory
//     not read".  In place under ONLY the whole tile is stored (flag lowered) unless it is flagged, paper is black and
//     no ink reaches it.
// WIDE: width % 4 == 0, z 16-byte and fb / out 4-byte aligned (the launcher checks): z in 16-byte pieces, a unit as three
// aligned words; otherwise the same through element accesses guarded by the width.  z, its flags, the winner words and
// the shadow buffer are only read.  No atomics, no inline assembly, no scratch.
constexpr int OUTLINE_LDS_W = TILE_W + 8, OUTLINE_LDS_H = TILE_H + 2 * (OUTLINE_MAX_RADIUS + 1);
constexpr int OUTLINE_SEED_H = TILE_H + 2 * OUTLINE_MAX_RADIUS, OUTLINE_SEED_WORDS = 3;  // rows of 192 bits, bit c = LDS column c
constexpr int OUTLINE_THREADS = 256, OUTLINE_UNITS = TILE_W * TILE_H / 4 / OUTLINE_THREADS;

template <bool WIDE>
__global__ __launch_bounds__(OUTLINE_THREADS) void k_outline(OutlineArgs a)
{
    static_assert(TILE_W == 128 && TILE_H == 16 && OUTLINE_UNITS == 2, "32 units to a row of a tile, two rounds of eight rows");
    static_assert(OUTLINE_MAX_RADIUS + 1 <= 4 && OUTLINE_MAX_RADIUS + 1 <= TILE_H, "the halo lies in the eight tiles around, within 4 columns");
    static_assert(OUTLINE_LDS_W <= 64 * OUTLINE_SEED_WORDS && OUTLINE_THREADS == 4 * 64, "three ballots cover a row; four waves");
    __shared__ float s_z[OUTLINE_LDS_H * OUTLINE_LDS_W];
    __shared__ unsigned long long s_seed[OUTLINE_SEED_H * OUTLINE_SEED_WORDS];
    const uint32_t t = blockIdx.x;
    const int32_t W = (int32_t)a.frame.width, H = (int32_t)a.frame.height, R = (int32_t)a.rule.radius;
    const int32_t ntx = (int32_t)a.frame.ntx, nty = (int32_t)a.frame.nty;
    const int32_t tx = (int32_t)t % ntx, ty = (int32_t)t / ntx;
    const int32_t x0 = tx * TILE_W, y0 = ty * TILE_H;
    const bool only = (a.rule.flags & OUTLINE_ONLY) != 0u, in_place = a.out == a.fb;
    const bool clean = a.fbclean[t] != 0u;  // (workgroup-uniform)
    // bit 3 * ay + ax: the tile at (tx + ax - 1, ty + ay - 1) reads as f32::MIN -- flag up, or no such tile
    uint32_t stale = 0u;
#pragma unroll
    for (int32_t ay = 0; ay < 3; ay++)
#pragma unroll
        for (int32_t ax = 0; ax < 3; ax++) {
            const int32_t nx = tx + ax - 1, ny = ty + ay - 1;
            bool up = nx < 0 || nx >= ntx || ny < 0 || ny >= nty;
            if (!up) up = a.zclean[ny * ntx + nx] != 0u;
            if (up) stale |= 1u << (3 * ay + ax);
        }
    // the units of k_grade
    const int32_t ux = 4 * (int32_t)(threadIdx.x % 32u), x = x0 + ux, row_first = (int32_t)(threadIdx.x / 32u);
    const int32_t n_px = min(4, W - x);  // (WIDE: 4, or the unit is outside)
    uint32_t inked[OUTLINE_UNITS];       // bit i: pixel i of the unit is inked
#pragma unroll
    for (int h = 0; h < OUTLINE_UNITS; h++) inked[h] = 0u;
    bool any_ink = false;
    if (stale != 0x1FFu) {  // (workgroup-uniform: the barriers are reached by all or none)
        const int32_t rows = TILE_H + 2 * (R + 1);  // LDS row r is frame row y0 - (R + 1) + r, LDS column c frame column x0 - 4 + c
        const float z_min = bits_f32(TR_F32_MIN_BITS);
        if (WIDE) {
            for (int32_t p = (int32_t)threadIdx.x; p < rows * (OUTLINE_LDS_W / 4); p += OUTLINE_THREADS) {
                const int32_t r = p / (OUTLINE_LDS_W / 4), j = p % (OUTLINE_LDS_W / 4);
                const int32_t px = x0 - 4 + 4 * j, py = y0 - (R + 1) + r;
                const int32_t ax = j < 1 ? 0 : j < 1 + TILE_W / 4 ? 1 : 2, ay = py < y0 ? 0 : py < y0 + TILE_H ? 1 : 2;
                float4 v = make_float4(z_min, z_min, z_min, z_min);
                if (((stale >> (3 * ay + ax)) & 1u) == 0u && px < W && py < H)
                    v = *reinterpret_cast<const float4 *>(a.z + (size_t)py * (size_t)W + (size_t)px);
                *reinterpret_cast<float4 *>(&s_z[r * OUTLINE_LDS_W + 4 * j]) = v;
            }
        } else {
            for (int32_t p = (int32_t)threadIdx.x; p < rows * OUTLINE_LDS_W; p += OUTLINE_THREADS) {
                const int32_t r = p / OUTLINE_LDS_W, c = p % OUTLINE_LDS_W;
                if (c < 3 - R || c > 4 + TILE_W + R) continue;  // (no pixel of the seed region looks at it)
                const int32_t px = x0 - 4 + c, py = y0 - (R + 1) + r;
                const int32_t ax = c < 4 ? 0 : c < 4 + TILE_W ? 1 : 2, ay = py < y0 ? 0 : py < y0 + TILE_H ? 1 : 2;
                float v = z_min;
                if (((stale >> (3 * ay + ax)) & 1u) == 0u && px < W && py < H) v = a.z[(size_t)py * (size_t)W + (size_t)px];
                s_z[r * OUTLINE_LDS_W + c] = v;
            }
        }
        __syncthreads();
        // seeds: seed row sr is frame row y0 - R + sr, LDS row sr + 1; bit c of a row is LDS column c
        const int32_t wave = (int32_t)(threadIdx.x / 64u), lane = (int32_t)(threadIdx.x % 64u);
        const int32_t seed_rows = TILE_H + 2 * R;
        for (int32_t task = wave; task < seed_rows * OUTLINE_SEED_WORDS; task += OUTLINE_THREADS / 64) {
            const int32_t sr = task / OUTLINE_SEED_WORDS, j = task % OUTLINE_SEED_WORDS;
            const int32_t c = 64 * j + lane, px = x0 - 4 + c, py = y0 - R + sr;
            bool seed = false;
            if (c >= 4 - R && c < 4 + TILE_W + R && px >= 0 && px < W && py >= 0 && py < H) {
                const float *q = s_z + (sr + 1) * OUTLINE_LDS_W + c;
                seed = outline_kinds(q[0], q[-1], q[1], q[-OUTLINE_LDS_W], q[OUTLINE_LDS_W], outline_exist(px, py, W, H), a.rule) != 0u;
            }
            const unsigned long long word = __ballot(seed ? 1 : 0);
            if (lane == 0) s_seed[sr * OUTLINE_SEED_WORDS + j] = word;
        }
        __syncthreads();
        // ink: the unit's window starts R bits left of its first pixel
        const int32_t first = 4 + ux - R, j = first >> 6, off = first & 63;
        const uint32_t span = (1u << (2 * R + 1)) - 1u;
        uint32_t mine = 0u;
#pragma unroll
        for (int h = 0; h < OUTLINE_UNITS; h++) {
            const int32_t row = row_first + 8 * h;  // seed rows row .. row + 2 R lie around it
            unsigned long long acc = 0ull;
            for (int32_t dy = 0; dy <= 2 * R; dy++) {
                const unsigned long long *w = s_seed + (row + dy) * OUTLINE_SEED_WORDS + j;
                acc |= w[0] >> off;
                if (off != 0 && j + 1 < OUTLINE_SEED_WORDS) acc |= w[1] << (64 - off);
            }
            const uint32_t window = (uint32_t)acc;
            const bool inside = x < W && y0 + row < H;
#pragma unroll
            for (int i = 0; i < 4; i++)
                if (inside && i < n_px && ((window >> i) & span) != 0u) inked[h] |= 1u << i;
            mine |= inked[h];
        }
        any_ink = __syncthreads_or((int)mine) != 0;
    }
    // what the tile needs (all workgroup-uniform)
    bool store_all = true, load = !only && !clean;
    if (in_place) {
        if (only) {
            if (clean && a.rule.paper == 0u && !any_ink) return;  // stays the cleared colour behind its flag
            load = false;
        } else {
            if (!any_ink) return;
            store_all = clean;  // zeros and ink over stale memory: every byte
        }
    }
    const uint32_t blank = only ? a.rule.paper : 0u;
#pragma unroll
    for (int h = 0; h < OUTLINE_UNITS; h++) {
        const int32_t y = y0 + row_first + 8 * h;
        if (x >= W || y >= H) continue;
        if (!store_all && inked[h] == 0u) continue;
        const size_t ci = ((size_t)(H - 1 - y) * (size_t)W + (size_t)x) * 3u;
        uint32_t px[4] = { blank, blank, blank, blank };
        if (load) {
            const uint8_t *q = a.fb + ci;
            if (WIDE) {
                const uint32_t *qw = reinterpret_cast<const uint32_t *>(q);
                const uint32_t w0 = qw[0], w1 = qw[1], w2 = qw[2];
                px[0] = w0 & 0xFFFFFFu;
                px[1] = (w0 >> 24) | ((w1 & 0xFFFFu) << 8);
                px[2] = (w1 >> 16) | ((w2 & 0xFFu) << 16);
                px[3] = w2 >> 8;
            } else {
#pragma unroll
                for (int i = 0; i < 4; i++)
                    if (i < n_px) px[i] = grade_pack(q[3 * i], q[3 * i + 1], q[3 * i + 2]);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; i++)
            if ((inked[h] >> i) & 1u) px[i] = outline_px(px[i], a.rule);
        uint8_t *o = a.out + ci;
        if (WIDE) {
            uint32_t *ow = reinterpret_cast<uint32_t *>(o);
            ow[0] = px[0] | (px[1] << 24);
            ow[1] = (px[1] >> 8) | (px[2] << 16);
            ow[2] = (px[2] >> 16) | (px[3] << 8);
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++)
                if (i < n_px) {
                    o[3 * i + 0] = (uint8_t)(px[i] & 0xFFu);
                    o[3 * i + 1] = (uint8_t)((px[i] >> 8) & 0xFFu);
                    o[3 * i + 2] = (uint8_t)((px[i] >> 16) & 0xFFu);
                }
        }
    }
    if (in_place && clean) {  // (workgroup-uniform) the tile's memory is its colour now
        __syncthreads();  // (every wave has read the flag)
        if (threadIdx.x == 0u) a.fbclean[t] = 0u;
    }
}

// Edge anti-aliasing (tr_scene_antialias): the frame's stair-steps smoothed by a luma-driven edge filter into `out`,
// never in place (a pixel reads lumas up to `search` pixels away and one neighbour's colour); tr_aa.h has the rule.  One
// workgroup of 256 lanes per 128 x 16 tile, the grid of k_bloom and k_outline.  The rule speaks of BUFFER rows (row 0 =
// top), so the kernel does too: tile row ty holds buffer rows by0 .. by0 + 15 with by0 = H - 16 - 16 ty (negative in a
// partial top row: those rows do not exist), and the tile row ABOVE it in the buffer is ty + 1.
//   * the nine colour flags of the 3 x 3 neighbourhood are workgroup-uniform (a tile outside the grid counts as up: what
//     is clamped from it repeats a border pixel of a tile inside).  All nine up: the tile is black and stays black,
//     nothing is read -- zeros are stored and, with out_clean, the output flag is raised (a raised colour flag says
//     "zeros, no need to load", and the memory behind it IS zeros: tr_scene_get_frame_buffer copies it as it lies);
//   * staging: the LUMA of the tile and a halo of `search` pixels goes to LDS as bytes, rows of 144 that start 8 pixels
//     left of the tile, so that a piece of four pixels (twelve bytes of the frame, one word of LDS) lies in ONE tile: a
//     piece behind a raised flag is zeros without a load.  What lies outside the frame is filled from LDS behind a
//     barrier with the luma of the clamped coordinates (only tiles whose halo leaves the frame take that pass);
//   * step 1 of the rule: a lane owns two units of four pixels, eight rows apart (k_outline's), and tests them from
//     three aligned words and two bytes of LDS a unit.  A pixel that passes goes onto a list in LDS (one LDS atomic a
//     lane for its place).  The list's length is the tile's vote: empty, and the tile is a copy of itself;
//   * steps 2 to 6: the list is dealt out to the lanes, 256 survivors at a time, so that the walk of the search runs on
//     full waves whatever the survivors' places are; a wave beyond the list's end does nothing.  The result (off and the
//     neighbour, 11 bits) goes to a u16 plane of the tile in LDS;
//   * output: a unit's twelve bytes are loaded (zeros behind the tile's own raised flag), a pixel with off > 0 fetches
//     its neighbour's three bytes straight from memory (zeros behind that tile's flag, the coordinates clamped) and
//     blends, every unit of the tile is stored;
//   * with out_clean a tile whose OWN flag is up votes (one barrier) whether any byte of its output is not zero -- colour
//     came in from a neighbour's edge: its output flag is 1 when none did (the zeros are stored all the same), else 0.
// LDS: 4608 + 4096 + 4096 bytes.  WIDE: width % 4 == 0 and fb / out 4-byte aligned (the launcher checks): a unit as
// three aligned words; otherwise the same through bytes guarded by the width.  fb and its flags are only read.  No
// global atomics, no inline assembly, no scratch.
constexpr int AA_LDS_W = TILE_W + 2 * AA_MAX_SEARCH, AA_LDS_H = TILE_H + 2 * AA_MAX_SEARCH;
constexpr int AA_THREADS = 256, AA_UNITS = TILE_W * TILE_H / 4 / AA_THREADS;

// L of the rule from the staged bytes: LDS row 0 is buffer row oy, LDS column 0 frame column ox.
struct AaTileLuma {
    const uint8_t *s;
    int32_t ox, oy;
    __device__ __forceinline__ int32_t operator()(int32_t x, int32_t y) const { return (int32_t)s[(y - oy) * AA_LDS_W + (x - ox)]; }
};

template <bool WIDE>
__global__ __launch_bounds__(AA_THREADS) void k_aa(AaArgs a)
{
    static_assert(TILE_W == 128 && TILE_H == 16 && AA_UNITS == 2, "32 units to a row of a tile, two rounds of eight rows");
    static_assert(AA_MAX_SEARCH % 4 == 0 && AA_MAX_SEARCH <= TILE_H && AA_LDS_W % 4 == 0, "the halo lies in the eight tiles around, in whole pieces");
    static_assert(TILE_W * TILE_H <= 65536, "a pixel's place in the tile fits a u16");
    __shared__ __align__(16) uint8_t s_l[AA_LDS_H * AA_LDS_W];
    __shared__ __align__(8) uint16_t s_found[TILE_W * TILE_H];
    __shared__ uint16_t s_list[TILE_W * TILE_H];
    __shared__ uint32_t s_n;
    const uint32_t t = blockIdx.x;
    const int32_t W = (int32_t)a.frame.width, H = (int32_t)a.frame.height, S = (int32_t)a.rule.search;
    const int32_t ntx = (int32_t)a.frame.ntx, nty = (int32_t)a.frame.nty;
    const int32_t tx = (int32_t)t % ntx, ty = (int32_t)t / ntx;
    const int32_t x0 = tx * TILE_W, by0 = H - TILE_H - ty * TILE_H;
    // bit 3 * ay + ax, the tile at (tx + ax - 1, ty + ay - 1): its colour reads as zeros (its flag is up), or no such tile
    uint32_t czero = 0u;
#pragma unroll
    for (int32_t ay = 0; ay < 3; ay++)
#pragma unroll
        for (int32_t ax = 0; ax < 3; ax++) {
            const int32_t nx = tx + ax - 1, ny = ty + ay - 1;
            const uint32_t bit = 1u << (3 * ay + ax);
            if (nx < 0 || nx >= ntx || ny < 0 || ny >= nty) czero |= bit;
            else if (a.fbclean != nullptr && a.fbclean[ny * ntx + nx] != 0u) czero |= bit;
        }
    const bool own_zero = (czero & (1u << 4)) != 0u;
    // the units of k_outline, in buffer rows
    const int32_t ux = 4 * (int32_t)(threadIdx.x % 32u), x = x0 + ux, row_first = (int32_t)(threadIdx.x / 32u);
    const int32_t n_px = min(4, W - x);  // (WIDE: 4, or the unit is outside)
    uint32_t px[AA_UNITS][4];
    if (czero == 0x1FFu) {  // (workgroup-uniform, ahead of the barriers)
        if (a.out_clean != nullptr && threadIdx.x == 0u) a.out_clean[t] = 1u;
#pragma unroll
        for (int h = 0; h < AA_UNITS; h++) {
            const int32_t by = by0 + row_first + 8 * h;
            if (x >= W || by < 0) continue;
            uint8_t *o = a.out + ((size_t)by * (size_t)W + (size_t)x) * 3u;
            if (WIDE) {
                uint32_t *ow = reinterpret_cast<uint32_t *>(o);
                ow[0] = 0u, ow[1] = 0u, ow[2] = 0u;
            } else {
                for (int32_t i = 0; i < 3 * n_px; i++) o[i] = 0u;
            }
        }
        return;
    }
    if (threadIdx.x == 0u) s_n = 0u;
    // staging, what lies in the frame: LDS row r is buffer row by0 - S + r, LDS column c frame column x0 - 8 + c
    const int32_t rows = TILE_H + 2 * S, c_first = AA_MAX_SEARCH - S, c_end = AA_MAX_SEARCH + TILE_W + S;
    if (WIDE) {
        for (int32_t p = (int32_t)threadIdx.x; p < rows * (AA_LDS_W / 4); p += AA_THREADS) {
            const int32_t r = p / (AA_LDS_W / 4), j = p % (AA_LDS_W / 4);
            if (4 * j + 3 < c_first || 4 * j >= c_end) continue;  // (no pixel of the tile looks at it)
            const int32_t qx = x0 - AA_MAX_SEARCH + 4 * j, qy = by0 - S + r;
            if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;  // (the clamp, below)
            const int32_t ax = j < AA_MAX_SEARCH / 4 ? 0 : j < (AA_MAX_SEARCH + TILE_W) / 4 ? 1 : 2;
            const int32_t ay = qy >= by0 + TILE_H ? 0 : qy >= by0 ? 1 : 2;
            uint32_t l4 = 0u;
            if (((czero >> (3 * ay + ax)) & 1u) == 0u) {
                // four pixels are twelve bytes at a multiple of four: three aligned words
                const uint32_t *q = reinterpret_cast<const uint32_t *>(a.fb + ((size_t)qy * (size_t)W + (size_t)qx) * 3u);
                const uint32_t w0 = q[0], w1 = q[1], w2 = q[2];
                l4 = aa_luma(w0 & 0xFFFFFFu) | (aa_luma((w0 >> 24) | ((w1 & 0xFFFFu) << 8)) << 8) |
                     (aa_luma((w1 >> 16) | ((w2 & 0xFFu) << 16)) << 16) | (aa_luma(w2 >> 8) << 24);
            }
            *reinterpret_cast<uint32_t *>(&s_l[r * AA_LDS_W + 4 * j]) = l4;
        }
    } else {
        for (int32_t p = (int32_t)threadIdx.x; p < rows * AA_LDS_W; p += AA_THREADS) {
            const int32_t r = p / AA_LDS_W, c = p % AA_LDS_W;
            if (c < c_first || c >= c_end) continue;
            const int32_t qx = x0 - AA_MAX_SEARCH + c, qy = by0 - S + r;
            if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
            const int32_t ax = c < AA_MAX_SEARCH ? 0 : c < AA_MAX_SEARCH + TILE_W ? 1 : 2;
            const int32_t ay = qy >= by0 + TILE_H ? 0 : qy >= by0 ? 1 : 2;
            uint32_t l = 0u;
            if (((czero >> (3 * ay + ax)) & 1u) == 0u) {
                const uint8_t *q = a.fb + ((size_t)qy * (size_t)W + (size_t)qx) * 3u;
                l = stats_luma(q[0], q[1], q[2]);
            }
            s_l[r * AA_LDS_W + c] = (uint8_t)l;
        }
    }
    // the clamp: what lies outside the frame repeats the border pixel, which the pass above has staged (the clamped
    // coordinates lie in the frame and between the tile and the place they are asked for)
    if (x0 - S < 0 || x0 + TILE_W + S > W || by0 - S < 0 || by0 + TILE_H + S > H) {  // (workgroup-uniform)
        __syncthreads();
        for (int32_t p = (int32_t)threadIdx.x; p < rows * AA_LDS_W; p += AA_THREADS) {
            const int32_t r = p / AA_LDS_W, c = p % AA_LDS_W;
            if (c < c_first || c >= c_end) continue;
            const int32_t qx = x0 - AA_MAX_SEARCH + c, qy = by0 - S + r;
            if (qx >= 0 && qx < W && qy >= 0 && qy < H) continue;
            const int32_t cx = aa_clamp(qx, W), cy = aa_clamp(qy, H);
            s_l[r * AA_LDS_W + c] = s_l[(cy - by0 + S) * AA_LDS_W + (cx - x0 + AA_MAX_SEARCH)];
        }
    }
    __syncthreads();
    // step 1 on the lane's eight pixels; the survivors go onto the list
    uint32_t passed = 0u;  // bit 4 * h + i: pixel i of unit h
#pragma unroll
    for (int h = 0; h < AA_UNITS; h++) {
        const int32_t row = row_first + 8 * h;
        if (x >= W || by0 + row < 0) continue;
        const uint8_t *base = s_l + (row + S) * AA_LDS_W + AA_MAX_SEARCH + ux;
        const uint32_t mid = *reinterpret_cast<const uint32_t *>(base);
        const uint32_t up = *reinterpret_cast<const uint32_t *>(base - AA_LDS_W), dn = *reinterpret_cast<const uint32_t *>(base + AA_LDS_W);
        // bytes 1..4 of `line` are the unit, byte 0 its left and byte 5 its right neighbour
        const unsigned long long line = (unsigned long long)base[-1] | ((unsigned long long)mid << 8) | ((unsigned long long)base[4] << 40);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            int32_t range = 0;
            const bool ok = aa_passes((int32_t)((mid >> (8 * i)) & 0xFFu), (int32_t)((up >> (8 * i)) & 0xFFu), (int32_t)((dn >> (8 * i)) & 0xFFu),
                                      (int32_t)((line >> (8 * i)) & 0xFFull), (int32_t)((line >> (8 * i + 16)) & 0xFFull), a.rule, &range);
            if (ok && i < n_px) passed |= 1u << (4 * h + i);
        }
        *reinterpret_cast<uint2 *>(&s_found[row * TILE_W + ux]) = make_uint2(0u, 0u);
    }
    if (passed != 0u) {
        uint32_t at = atomicAdd(&s_n, (uint32_t)__popc(passed));  // (LDS; the order of the list does not matter)
#pragma unroll
        for (int k = 0; k < 4 * AA_UNITS; k++)
            if ((passed >> k) & 1u) s_list[at++] = (uint16_t)((row_first + 8 * (k / 4)) * TILE_W + ux + (k % 4));
    }
    __syncthreads();
    const uint32_t n = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_n);
    // steps 2 to 6 on the survivors, a lane each
    if (n != 0u) {  // (workgroup-uniform)
        const AaTileLuma L = { s_l, x0 - AA_MAX_SEARCH, by0 - S };
        for (uint32_t k = threadIdx.x; k < n; k += AA_THREADS) {
            const int32_t at = (int32_t)s_list[k], lx = at % TILE_W, lr = at / TILE_W;
            const int32_t gx = x0 + lx, gy = by0 + lr;
            int32_t range = 0;
            (void)aa_passes(L(gx, gy), L(gx, gy - 1), L(gx, gy + 1), L(gx - 1, gy), L(gx + 1, gy), a.rule, &range);
            s_found[at] = (uint16_t)aa_found(L, gx, gy, range, a.rule);
        }
        __syncthreads();
    }
    // output
    uint32_t lit = 0u;  // the tile's output bytes, or-ed
#pragma unroll
    for (int h = 0; h < AA_UNITS; h++) {
        const int32_t row = row_first + 8 * h, by = by0 + row;
#pragma unroll
        for (int i = 0; i < 4; i++) px[h][i] = 0u;
        if (x >= W || by < 0) continue;
        const size_t ci = ((size_t)by * (size_t)W + (size_t)x) * 3u;
        if (!own_zero) {
            const uint8_t *q = a.fb + ci;
            if (WIDE) {
                const uint32_t *qw = reinterpret_cast<const uint32_t *>(q);
                const uint32_t w0 = qw[0], w1 = qw[1], w2 = qw[2];
                px[h][0] = w0 & 0xFFFFFFu;
                px[h][1] = (w0 >> 24) | ((w1 & 0xFFFFu) << 8);
                px[h][2] = (w1 >> 16) | ((w2 & 0xFFu) << 16);
                px[h][3] = w2 >> 8;
            } else {
#pragma unroll
                for (int i = 0; i < 4; i++)
                    if (i < n_px) px[h][i] = grade_pack(q[3 * i], q[3 * i + 1], q[3 * i + 2]);
            }
        }
        const uint2 f2 = *reinterpret_cast<const uint2 *>(&s_found[row * TILE_W + ux]);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t found = ((i < 2 ? f2.x : f2.y) >> (16 * (i % 2))) & 0xFFFFu;
            const uint32_t off = found & AA_OFF_MASK, to = found >> 9;
            uint32_t fn = 0u;
            if (off != 0u && (a.rule.flags & AA_SHOW_BLEND) == 0u) {
                // p + n clamped to the frame; its tile is one of the nine
                const int32_t cx = aa_clamp(x + i + aa_dx(to), W), cy = aa_clamp(by + aa_dy(to), H);
                const int32_t ax = cx / TILE_W - tx + 1, ay = (H - 1 - cy) / TILE_H - ty + 1;
                if (((czero >> (3 * ay + ax)) & 1u) == 0u) {
                    const uint8_t *q = a.fb + ((size_t)cy * (size_t)W + (size_t)cx) * 3u;
                    fn = grade_pack(q[0], q[1], q[2]);
                }
            }
            if (i < n_px) px[h][i] = aa_out_px(px[h][i], fn, off, a.rule);
            lit |= px[h][i];
        }
    }
    if (a.out_clean != nullptr) {  // (workgroup-uniform) behind its own flag: did colour come in from a neighbour's edge?
        const bool any_lit = !own_zero || __syncthreads_or((int)lit) != 0;
        if (threadIdx.x == 0u) a.out_clean[t] = any_lit ? 0u : 1u;
    }
#pragma unroll
    for (int h = 0; h < AA_UNITS; h++) {
        const int32_t by = by0 + row_first + 8 * h;
        if (x >= W || by < 0) continue;
        uint8_t *o = a.out + ((size_t)by * (size_t)W + (size_t)x) * 3u;
        if (WIDE) {
            uint32_t *ow = reinterpret_cast<uint32_t *>(o);
            ow[0] = px[h][0] | (px[h][1] << 24);
            ow[1] = (px[h][1] >> 8) | (px[h][2] << 16);
            ow[2] = (px[h][2] >> 16) | (px[h][3] << 8);
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++)
                if (i < n_px) {
                    o[3 * i + 0] = (uint8_t)(px[h][i] & 0xFFu);
                    o[3 * i + 1] = (uint8_t)((px[h][i] >> 8) & 0xFFu);
                    o[3 * i + 2] = (uint8_t)((px[h][i] >> 16) & 0xFFu);
                }
        }
    }
}

// Resize (tr_scene_resize): the frame scaled to out_w x out_h by the separable integer filter of tr_resize.h.  The rule's
// divisions were done on the host; the kernel gets, per axis, first index | count << 16 and RESIZE_MAX_TAPS u16 weights
// to an output index, and multiplies and adds in u32.  One workgroup of 256 lanes per tile of OTW x OTH OUTPUT pixels
// (kResizeShapes: the launcher's caller chose the shape so that the source rows a tile's OTH rows reach over are at most
// ROWS).  Everything is in BUFFER rows (row 0 = top); source tile row ty is buffer rows H - 16 - 16 ty onwards.
//   * footprint: the tile's source columns and rows from the tables' first and last entries (the runs move monotonically),
//     the colour flags of the 128 x 16 source tiles it touches to LDS -- at most 6 x 5 of them -- and one vote: all up,
//     and the tile is stored as zeros without a load;
//   * phase 1: a lane owns ONE output column of the tile -- its run's weights stay in registers, two 16-byte loads --
//     and walks the footprint's source rows 256 / OTW apart: the run's pixels from memory as bytes, the part of the run
//     behind a raised flag contributing zeros without a load (a run of at most 16 pixels lies in at most two source
//     tiles), three unrounded u32 sums to LDS, row-major, 3 OTW words a row;
//   * phase 2: a lane per output BYTE (row, 3 x + c): consecutive lanes read consecutive words of LDS, the row's
//     weights come from LDS; round, shift, and the byte goes to a staging tile in LDS;
//   * stores from the staging tile: 12-byte units of four pixels as three aligned words where WIDE (out_w % 4 == 0 and
//     `out` 4-byte aligned: the launcher checks), otherwise bytes, consecutive lanes consecutive bytes, guarded by the
//     output's width and height.  Every byte of `out` is written.
// LDS: ROWS * OTW * 12 + OTW * OTH * 3 + OTH * (32 + 4) + 128 bytes.  No global atomics, no inline assembly, no scratch.
constexpr int RESIZE_THREADS = 256, RESIZE_FLAGS_W = 6, RESIZE_FLAGS_H = 5;

template <int OTW, int OTH, int ROWS, bool WIDE>
__global__ __launch_bounds__(RESIZE_THREADS) void k_resize(ResizeArgs a)
{
    static_assert(RESIZE_THREADS % OTW == 0 && OTW % 4 == 0 && OTW * OTH / 4 <= RESIZE_THREADS, "a lane keeps its column; a unit a lane at most");
    static_assert((OTW - 1) * 8 + 1 + RESIZE_MAX_TAPS <= (RESIZE_FLAGS_W - 1) * TILE_W + 1 && ROWS <= (RESIZE_FLAGS_H - 1) * TILE_H + 1,
                  "the footprint's source tiles fit the flag array");
    static_assert(OTH * RESIZE_MAX_TAPS <= RESIZE_THREADS && RESIZE_FLAGS_W * RESIZE_FLAGS_H <= RESIZE_THREADS, "one lane a weight, one a flag");
    __shared__ uint32_t s_sum[ROWS * OTW * 3];
    __shared__ __align__(4) uint8_t s_out[OTH * OTW * 3];
    __shared__ uint16_t s_wy[OTH * RESIZE_MAX_TAPS];
    __shared__ uint32_t s_fcy[OTH];
    __shared__ uint32_t s_zero[RESIZE_FLAGS_W * RESIZE_FLAGS_H];
    const int32_t W = (int32_t)a.frame.width, H = (int32_t)a.frame.height, ntx = (int32_t)a.frame.ntx;
    const int32_t Wd = (int32_t)a.out_w, Hd = (int32_t)a.out_h;
    const int32_t X0 = (int32_t)blockIdx.x * OTW, Y0 = (int32_t)blockIdx.y * OTH;
    const int32_t n_x = min(OTW, Wd - X0), n_y = min(OTH, Hd - Y0);  // the tile's columns and rows inside the output (>= 1)
    // the footprint (workgroup-uniform): source columns [sx0, sx1], buffer rows [sy0, sy1]
    const uint32_t fx_a = a.x.fc[X0], fx_b = a.x.fc[X0 + n_x - 1], fy_a = a.y.fc[Y0], fy_b = a.y.fc[Y0 + n_y - 1];
    const int32_t sx0 = (int32_t)(fx_a & 0xFFFFu), sx1 = (int32_t)(fx_b & 0xFFFFu) + (int32_t)(fx_b >> 16) - 1;
    const int32_t sy0 = (int32_t)(fy_a & 0xFFFFu), sy1 = (int32_t)(fy_b & 0xFFFFu) + (int32_t)(fy_b >> 16) - 1;
    const int32_t n_rows = min(sy1 - sy0 + 1, ROWS);  // (the shape was chosen so that the min changes nothing)
    // its source tiles: columns ftx0 .. ftx1, tile rows fty0 (of buffer row sy1, the lowest) .. fty1
    const int32_t ftx0 = sx0 / TILE_W, ftx1 = sx1 / TILE_W, fty0 = (H - 1 - sy1) / TILE_H, fty1 = (H - 1 - sy0) / TILE_H;
    const int32_t fw = ftx1 - ftx0 + 1, fh = fty1 - fty0 + 1;
    bool up = true;
    if ((int32_t)threadIdx.x < fw * fh) {  // (fw <= RESIZE_FLAGS_W, fh <= RESIZE_FLAGS_H: the launcher checks the spans)
        const int32_t fx = (int32_t)threadIdx.x % fw, fy = (int32_t)threadIdx.x / fw;
        up = a.fbclean != nullptr && a.fbclean[(fty0 + fy) * ntx + ftx0 + fx] != 0u;
        s_zero[fy * RESIZE_FLAGS_W + fx] = up ? 1u : 0u;
    }
    if ((int32_t)threadIdx.x < n_y * RESIZE_MAX_TAPS)
        s_wy[threadIdx.x] = a.y.w[(size_t)Y0 * RESIZE_MAX_TAPS + threadIdx.x];
    if ((int32_t)threadIdx.x < n_y) s_fcy[threadIdx.x] = a.y.fc[Y0 + (int32_t)threadIdx.x];
    const bool zeros = __syncthreads_and((int)up) != 0;  // (also the barrier behind the three arrays)
    if (!zeros) {  // (workgroup-uniform)
        // phase 1
        const int32_t lx = (int32_t)threadIdx.x % OTW;
        if (lx < n_x) {
            const uint32_t fc = a.x.fc[X0 + lx];
            const int32_t x0 = (int32_t)(fc & 0xFFFFu), n = (int32_t)(fc >> 16);
            const uint4 *wp = reinterpret_cast<const uint4 *>(a.x.w + (size_t)(X0 + lx) * RESIZE_MAX_TAPS);
            const uint4 wa = wp[0], wb = wp[1];
            const uint32_t w2[RESIZE_MAX_TAPS / 2] = { wa.x, wa.y, wa.z, wa.w, wb.x, wb.y, wb.z, wb.w };
            // the run lies in source tile column x0 / 128 up to `split`, in the next one from there
            const int32_t fc0 = x0 / TILE_W - ftx0, split = (x0 / TILE_W + 1) * TILE_W;
            const int32_t fc1 = (x0 + n - 1) / TILE_W - ftx0;
            for (int32_t r = (int32_t)threadIdx.x / OTW; r < n_rows; r += RESIZE_THREADS / OTW) {
                const int32_t sy = sy0 + r, fr = ((H - 1 - sy) / TILE_H - fty0) * RESIZE_FLAGS_W;
                const bool z0 = s_zero[fr + fc0] != 0u, z1 = s_zero[fr + fc1] != 0u;
                uint32_t acc0 = 0u, acc1 = 0u, acc2 = 0u;
                if (!(z0 && z1)) {
                    const uint8_t *p = a.fb + ((size_t)sy * (size_t)W + (size_t)x0) * 3u;
#pragma unroll
                    for (int k = 0; k < RESIZE_MAX_TAPS; k++) {
                        if (k >= n) break;
                        const uint32_t w = (w2[k / 2] >> (16 * (k % 2))) & 0xFFFFu;
                        if (x0 + k < split ? z0 : z1) continue;
                        acc0 += w * (uint32_t)p[3 * k + 0];
                        acc1 += w * (uint32_t)p[3 * k + 1];
                        acc2 += w * (uint32_t)p[3 * k + 2];
                    }
                }
                uint32_t *d = &s_sum[(r * OTW + lx) * 3];
                d[0] = acc0, d[1] = acc1, d[2] = acc2;
            }
        }
        __syncthreads();
        // phase 2
        for (int32_t v = (int32_t)threadIdx.x; v < n_y * OTW * 3; v += RESIZE_THREADS) {
            const int32_t ly = v / (OTW * 3), j = v % (OTW * 3);
            if (j >= n_x * 3) continue;
            const uint32_t fc = s_fcy[ly];
            const int32_t r0 = (int32_t)(fc & 0xFFFFu) - sy0, n = (int32_t)(fc >> 16);
            uint32_t acc = 1u << 23;
            for (int32_t k = 0; k < n; k++) acc += (uint32_t)s_wy[ly * RESIZE_MAX_TAPS + k] * s_sum[min(r0 + k, n_rows - 1) * (OTW * 3) + j];
            s_out[ly * (OTW * 3) + j] = (uint8_t)(acc >> 24);
        }
        __syncthreads();
    }
    // stores
    if (WIDE) {
        const int32_t u = (int32_t)threadIdx.x, ly = u / (OTW / 4), ux = 4 * (u % (OTW / 4));
        if (ly < n_y && ux < n_x) {  // (out_w % 4 == 0: a unit lies inside the output or outside it)
            const uint32_t *q = reinterpret_cast<const uint32_t *>(&s_out[ly * (OTW * 3) + ux * 3]);
            uint32_t *o = reinterpret_cast<uint32_t *>(a.out + ((size_t)(Y0 + ly) * (size_t)Wd + (size_t)(X0 + ux)) * 3u);
            o[0] = zeros ? 0u : q[0], o[1] = zeros ? 0u : q[1], o[2] = zeros ? 0u : q[2];
        }
    } else {
        for (int32_t v = (int32_t)threadIdx.x; v < n_y * OTW * 3; v += RESIZE_THREADS) {
            const int32_t ly = v / (OTW * 3), j = v % (OTW * 3);
            if (j >= n_x * 3) continue;
            a.out[((size_t)(Y0 + ly) * (size_t)Wd + (size_t)X0) * 3u + (size_t)j] = zeros ? (uint8_t)0u : s_out[ly * (OTW * 3) + j];
        }
    }
}

// Warp (tr_scene_warp): the frame resampled to out_w x out_h through a grid of source coordinates; tr_warp.h has the
// rule.  One workgroup of 256 lanes per tile of 128 x 16 OUTPUT pixels: eight grid cells in a row, so a tile owns whole
// cells and, where the output has the frame's size and a height that is a multiple of 16, is a tile of the frame's
// grid.  Everything is in BUFFER rows (row 0 = top); source tile row ty is buffer rows H - 16 - 16 ty onwards.
//   * nodes: the tile's 9 x 2 nodes of each grid to LDS (a partial tile repeats the last node of its last cell);
//   * footprint (workgroup-uniform): a pixel's coordinate is a convex combination of its cell's nodes, so the tile's
//     texels lie in [min >> 8, (max >> 8) + 1] per axis over those nodes.  Wholly outside the image under WARP_BORDER:
//     the tile is the border colour.  Otherwise the colour flags of the 128 x 16 source tiles under the footprint,
//     clamped to the image -- a lane every 256th, up to WARP_FLAG_TILES of them, beyond which nothing is concluded --
//     and two votes: ALL up and the rule gives black there (WARP_CLAMP, a border of 0, or a footprint wholly inside):
//     the tile is stored as zeros without a load; NONE up: no texel asks for its flag;
//   * gather: a lane owns one column of the tile and every other row, eight pixels: coordinates from the nodes in LDS,
//     four texels straight from memory through L1 / L2 as bytes -- a texel of weight 0 is skipped, one outside the image is
//     the border or clamped, one behind a raised flag is zero WITHOUT a load (its memory is stale) --, the rounded bytes
//     to a staging tile in LDS.  PC (WARP_PER_CHANNEL): three coordinates a pixel, one byte a texel;
//   * stores from the staging tile (or the constant): 12-byte units of four pixels as three aligned words where WIDE
//     (out_w % 4 == 0 and `out` 4-byte aligned: the launcher checks), otherwise bytes, consecutive lanes consecutive
//     bytes, guarded by the output's width and height.  Every byte of `out` is written;
//   * out_clean, when given, gets the tile's flag: 1 where the tile was stored as zeros without a load, else 0.
// LDS: 6144 bytes of staging and 144 (PC: 432) of nodes.  No atomics, no inline assembly, no scratch.
constexpr int WARP_THREADS = 256, WARP_TW = TILE_W, WARP_TH = WARP_CELL, WARP_NODES_X = WARP_TW / WARP_CELL + 1;
constexpr int WARP_ROWS = WARP_TW * WARP_TH / WARP_THREADS;  // pixels of its column a lane owns
constexpr int32_t WARP_FLAG_TILES = 1024;  // (four flags a lane)

// One sample of the rule at (sx, sy): all three channels into o, or (PC) channel ch alone.
template <bool PC>
__device__ __forceinline__ void warp_sample(const WarpArgs &a, int32_t W, int32_t H, int32_t ntx, bool any_up, int32_t sx, int32_t sy,
                                            int ch, uint32_t (&o)[3])
{
    const int32_t ix = sx >> 8, iy = sy >> 8;
    const WarpWeights w = warp_weights((uint32_t)(sx & 255), (uint32_t)(sy & 255));
    const uint32_t wt[4] = { w.w00, w.w10, w.w01, w.w11 };
    uint32_t sum[3] = { 0u, 0u, 0u };
#pragma unroll
    for (int t = 0; t < 4; t++) {
        if (wt[t] == 0u) continue;
        int32_t x = ix + (t & 1), y = iy + (t >> 1);
        bool in = x >= 0 && x < W && y >= 0 && y < H;
        if (a.rule.edge == WARP_CLAMP) {
            x = min(max(x, 0), W - 1), y = min(max(y, 0), H - 1);
            in = true;
        }
        uint32_t v[3] = { a.rule.border[0], a.rule.border[1], a.rule.border[2] };
        if (in) {  // (x, y) lies in the image from here on
            if (any_up && a.fbclean[((H - 1 - y) / TILE_H) * ntx + x / TILE_W] != 0u) {
                v[0] = v[1] = v[2] = 0u;
            } else {
                const uint8_t *p = a.fb + ((size_t)y * (size_t)W + (size_t)x) * 3u;
                if (PC) v[ch] = p[ch];
                else v[0] = p[0], v[1] = p[1], v[2] = p[2];
            }
        }
        if (PC) sum[ch] += wt[t] * v[ch];
        else sum[0] += wt[t] * v[0], sum[1] += wt[t] * v[1], sum[2] += wt[t] * v[2];
    }
    if (PC) o[ch] = warp_round(sum[ch]);
    else o[0] = warp_round(sum[0]), o[1] = warp_round(sum[1]), o[2] = warp_round(sum[2]);
}

template <bool PC, bool WIDE>
__global__ __launch_bounds__(WARP_THREADS) void k_warp(WarpArgs a)
{
    constexpr int NG = PC ? 3 : 1, NODES = NG * 2 * WARP_NODES_X;
    static_assert(WARP_TW == 128 && WARP_TH == 16 && WARP_TH == TILE_H && NODES <= WARP_THREADS, "a tile of the frame's grid, one cell tall; a lane a node");
    static_assert(WARP_THREADS % WARP_TW == 0 && WARP_TW * WARP_TH / 4 == 2 * WARP_THREADS, "a lane keeps its column; two units a lane");
    __shared__ int32_t s_node[NODES * 2];
    __shared__ __align__(4) uint8_t s_out[WARP_TH * WARP_TW * 3];
    const int32_t W = (int32_t)a.frame.width, H = (int32_t)a.frame.height, ntx = (int32_t)a.frame.ntx, nty = (int32_t)a.frame.nty;
    const int32_t Wd = (int32_t)a.out_w, Hd = (int32_t)a.out_h;
    const int32_t gw = (int32_t)warp_grid_side(a.out_w), gh = (int32_t)warp_grid_side(a.out_h);
    const int32_t bx = (int32_t)blockIdx.x, by = (int32_t)blockIdx.y;
    const int32_t X0 = bx * WARP_TW, Y0 = by * WARP_TH;
    const int32_t n_x = min(WARP_TW, Wd - X0), n_y = min(WARP_TH, Hd - Y0);  // the tile's columns and rows inside the output (>= 1)
    const int32_t n_cx = (n_x + WARP_CELL - 1) / WARP_CELL;                   // its cells inside the output: nodes 0 .. n_cx
    if ((int32_t)threadIdx.x < NODES) {
        const int32_t g = (int32_t)threadIdx.x / (2 * WARP_NODES_X), r = (int32_t)threadIdx.x / WARP_NODES_X % 2;
        const int32_t c = min((int32_t)threadIdx.x % WARP_NODES_X, n_cx);
        // (column bx * 8 + n_cx <= gw - 1 and row by + 1 <= gh - 1: the grid has a node behind the last cell)
        const size_t at = (size_t)g * (size_t)(gw * gh) + (size_t)(by + r) * (size_t)gw + (size_t)(bx * (WARP_NODES_X - 1) + c);
        const int2 v = reinterpret_cast<const int2 *>(a.grid)[at];
        s_node[2 * threadIdx.x] = v.x, s_node[2 * threadIdx.x + 1] = v.y;
    }
    __syncthreads();
    // the footprint (workgroup-uniform): source columns [fx0, fx1], buffer rows [fy0, fy1], maybe outside the image
    int32_t lo_x = s_node[0], hi_x = lo_x, lo_y = s_node[1], hi_y = lo_y;
    for (int i = 1; i < NODES; i++) {
        const int32_t x = s_node[2 * i], y = s_node[2 * i + 1];
        lo_x = min(lo_x, x), hi_x = max(hi_x, x), lo_y = min(lo_y, y), hi_y = max(hi_y, y);
    }
    const int32_t fx0 = lo_x >> 8, fx1 = (hi_x >> 8) + 1, fy0 = lo_y >> 8, fy1 = (hi_y >> 8) + 1;
    const bool outside = fx1 < 0 || fx0 >= W || fy1 < 0 || fy0 >= H;
    const bool inside = fx0 >= 0 && fx1 < W && fy0 >= 0 && fy1 < H;
    const bool border_mode = a.rule.edge != WARP_CLAMP;
    const uint32_t br = a.rule.border[0], bg = a.rule.border[1], bb = a.rule.border[2];
    bool constant = false, any_up = false;
    uint32_t cr = 0u, cg = 0u, cb = 0u;  // the constant tile's colour
    if (border_mode && outside) {
        constant = true, cr = br, cg = bg, cb = bb;
    } else if (a.fbclean != nullptr) {
        // the source tiles under the footprint clamped to the image: columns ftx0 .. ftx1, tile rows fty0 .. fty1
        const int32_t cx0 = min(max(fx0, 0), W - 1), cx1 = min(max(fx1, 0), W - 1), cy0 = min(max(fy0, 0), H - 1), cy1 = min(max(fy1, 0), H - 1);
        const int32_t ftx0 = cx0 / TILE_W, ftx1 = cx1 / TILE_W, fty0 = (H - 1 - cy1) / TILE_H, fty1 = (H - 1 - cy0) / TILE_H;
        const int32_t fw = ftx1 - ftx0 + 1, n_ft = fw * (fty1 - fty0 + 1);
        if (n_ft <= WARP_FLAG_TILES) {
            bool up = true, down = true;
            for (int32_t i = (int32_t)threadIdx.x; i < n_ft; i += WARP_THREADS) {
                const bool f = a.fbclean[(fty0 + i / fw) * ntx + ftx0 + i % fw] != 0u;
                up = up && f, down = down && !f;
            }
            const bool all_up = __syncthreads_and((int)up) != 0;
            any_up = __syncthreads_and((int)down) == 0;
            if (all_up && (!border_mode || (br | bg | bb) == 0u || inside)) constant = true;
        } else {
            any_up = true;
        }
    }
    if (a.out_clean != nullptr && threadIdx.x == 0u)  // (the launcher: the output's tiles are the frame's)
        a.out_clean[(nty - 1 - by) * ntx + bx] = (constant && (cr | cg | cb) == 0u) ? 1u : 0u;
    if (!constant) {  // (workgroup-uniform)
        const int32_t lx = (int32_t)threadIdx.x % WARP_TW, cell = lx / WARP_CELL, fx = lx % WARP_CELL;
        if (lx < n_x) {
#pragma unroll 2
            for (int k = 0; k < WARP_ROWS; k++) {
                const int32_t ly = (int32_t)threadIdx.x / WARP_TW + (WARP_THREADS / WARP_TW) * k;  // (= Y & 15: the tile is one cell tall)
                if (ly >= n_y) break;
                uint32_t o[3];
#pragma unroll
                for (int g = 0; g < NG; g++) {
                    const int32_t *n0 = &s_node[(g * 2 * WARP_NODES_X + cell) * 2], *n1 = n0 + WARP_NODES_X * 2;
                    const int32_t sx = warp_coord(n0[0], n0[2], n1[0], n1[2], fx, ly);
                    const int32_t sy = warp_coord(n0[1], n0[3], n1[1], n1[3], fx, ly);
                    warp_sample<PC>(a, W, H, ntx, any_up, sx, sy, g, o);
                }
                uint8_t *d = &s_out[(ly * WARP_TW + lx) * 3];
                d[0] = (uint8_t)o[0], d[1] = (uint8_t)o[1], d[2] = (uint8_t)o[2];
            }
        }
        __syncthreads();
    }
    // stores
    if (WIDE) {
        // four pixels of the constant colour as three words: r g b r | g b r g | b r g b
        const uint32_t k0 = cr | (cg << 8) | (cb << 16) | (cr << 24), k1 = cg | (cb << 8) | (cr << 16) | (cg << 24);
        const uint32_t k2 = cb | (cr << 8) | (cg << 16) | (cb << 24);
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int32_t u = (int32_t)threadIdx.x + WARP_THREADS * j, ly = u / (WARP_TW / 4), ux = 4 * (u % (WARP_TW / 4));
            if (ly < n_y && ux < n_x) {  // (out_w % 4 == 0: a unit lies inside the output or outside it)
                const uint32_t *q = reinterpret_cast<const uint32_t *>(&s_out[(ly * WARP_TW + ux) * 3]);
                uint32_t *o = reinterpret_cast<uint32_t *>(a.out + ((size_t)(Y0 + ly) * (size_t)Wd + (size_t)(X0 + ux)) * 3u);
                o[0] = constant ? k0 : q[0], o[1] = constant ? k1 : q[1], o[2] = constant ? k2 : q[2];
            }
        }
    } else {
        for (int32_t v = (int32_t)threadIdx.x; v < n_y * WARP_TW * 3; v += WARP_THREADS) {
            const int32_t ly = v / (WARP_TW * 3), j = v % (WARP_TW * 3);
            if (j >= n_x * 3) continue;
            const uint32_t k = j % 3 == 0 ? cr : (j % 3 == 1 ? cg : cb);
            a.out[((size_t)(Y0 + ly) * (size_t)Wd + (size_t)X0) * 3u + (size_t)j] = constant ? (uint8_t)k : s_out[ly * (WARP_TW * 3) + j];
        }
    }
}

// YUV output (tr_scene_to_yuv, tr_scene_to_yuv_from): an rgb8 image converted to YCbCr planes by the rule of tr_yuv.h.
// Pointwise and memory-bound: 3 bytes a pixel in, 1.5 (4:2:0) or 3 (4:4:4) out, no LDS, no barrier, no atomics.  One
// workgroup per block of 128 columns x 16 BUFFER rows counted from the TOP (rows 16 by .. 16 by + 15), not per tile of the
// flag grid, which counts from the bottom: a chroma sample's two rows 2j and 2j + 1 then always lie in one workgroup, at
// every height.  One workgroup a block and no persistent walk: a workgroup has no table to stage and no setup to spread
// over several tiles (k_grade's reason), so a walk would only add its loop.
//   * unit: a lane converts N columns x 2 rows, N / 2 chroma samples of 4:2:0: N = 8 where width % 8 == 0 and src and out
//     are 8-byte aligned (three 8-byte loads a row; 8-byte stores of Y, of NV12's pairs and of I444's chroma, 4-byte
//     stores of I420's chroma), N = 4 where width % 4 == 0 and both are 4-byte aligned (three 4-byte loads a row; 4-byte
//     stores, 2-byte stores of I420's chroma), N = 2 with byte loads and byte stores otherwise -- any width, any address:
//     the chroma planes begin at out + W H, odd whenever W H is.  In the two wide forms every plane's offset and row
//     length is a multiple of the store's size (W H, cw = W / 2 and cw ch are); a unit lies inside the image or outside.
//   * flags: a workgroup's columns are those of ONE column of flag tiles; its rows lie in at most TWO tile rows, ty_top =
//     (H - 1 - 16 by) / 16 and the one below it, whose border is buffer row H - 16 ty_top.  With an even H that border is
//     even and a chroma pair (2j, 2j + 1) has both rows in one tile.  With an odd H EVERY border falls between the two
//     rows of a pair: row 2j is the last of the upper tile, 2j + 1 the first of the lower.  So the flag is taken per ROW:
//     a row behind a raised flag is not loaded and counts as zeros -- its Y is y0, and it adds nothing to the pair's sums.
//     Both rows flagged: Y = y0 and chroma 128 without a load.  clean == null: every row is read.
//   * odd edges (N = 2 only for columns, every N for rows): column min(x + 1, W - 1) and row min(y + 1, H - 1) are counted
//     twice from the values already loaded; their Y is not stored.
// Every byte of `out` is written, none outside.  No depth is read.
constexpr int YUV_BW = 128, YUV_BH = 16;

template <int N>
__device__ __forceinline__ void yuv_load_row(const uint8_t *p, bool second_column, uint32_t (&w)[6])
{
    if (N == 8) {
        const uint2 *q = reinterpret_cast<const uint2 *>(p);
        const uint2 a = q[0], b = q[1], c = q[2];
        w[0] = a.x, w[1] = a.y, w[2] = b.x, w[3] = b.y, w[4] = c.x, w[5] = c.y;
    } else if (N == 4) {
        const uint32_t *q = reinterpret_cast<const uint32_t *>(p);
        w[0] = q[0], w[1] = q[1], w[2] = q[2];
    } else {
        const uint8_t *s = second_column ? p + 3 : p;  // (the last column twice at an odd width)
        w[0] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)s[0] << 24);
        w[1] = (uint32_t)s[1] | ((uint32_t)s[2] << 8);
    }
}

// Byte k of a row's words (k is a constant after unrolling).
__device__ __forceinline__ int32_t yuv_byte(const uint32_t (&w)[6], int k) { return (int32_t)((w[k >> 2] >> (8 * (k & 3))) & 0xFFu); }

// n bytes (n = 8, 4, 2: one aligned store; the caller has seen to the alignment) from lo and hi.
template <int BYTES>
__device__ __forceinline__ void yuv_store(uint8_t *p, uint32_t lo, uint32_t hi)
{
    if (BYTES == 8) *reinterpret_cast<uint2 *>(p) = make_uint2(lo, hi);
    else if (BYTES == 4) *reinterpret_cast<uint32_t *>(p) = lo;
    else *reinterpret_cast<uint16_t *>(p) = (uint16_t)lo;
}

template <int N, uint32_t LAYOUT>
__global__ __launch_bounds__(256) void k_yuv(YuvArgs a)
{
    static_assert(N == 8 || N == 4 || N == 2, "a unit is 8, 4 or 2 columns");
    constexpr int UNITS_X = YUV_BW / N, UNITS = UNITS_X * (YUV_BH / 2);
    const int32_t W = (int32_t)a.width, H = (int32_t)a.height;
    const int32_t cw = (W + 1) / 2, ch = (H + 1) / 2;
    const size_t wh = (size_t)W * (size_t)H;
    const YuvRule k = a.rule;
    // the two flags this workgroup's rows can lie behind (workgroup-uniform)
    const int32_t ty_top = (H - 1 - (int32_t)blockIdx.y * YUV_BH) / TILE_H;
    bool up_top = false, up_low = false;
    if (a.clean != nullptr) {
        up_top = a.clean[(size_t)ty_top * a.ntx + blockIdx.x] != 0u;
        up_low = ty_top >= 1 ? a.clean[(size_t)(ty_top - 1) * a.ntx + blockIdx.x] != 0u : up_top;
    }
    for (int32_t u = (int32_t)threadIdx.x; u < UNITS; u += (int32_t)blockDim.x) {
        const int32_t x = (int32_t)blockIdx.x * YUV_BW + (u % UNITS_X) * N;
        const int32_t y0 = (int32_t)blockIdx.y * YUV_BH + (u / UNITS_X) * 2;
        if (x >= W || y0 >= H) continue;
        const bool row1 = y0 + 1 < H, col1 = x + 1 < W;  // (col1 matters where N == 2)
        const int32_t y1 = row1 ? y0 + 1 : y0;
        const bool z0 = (H - 1 - y0) / TILE_H == ty_top ? up_top : up_low;
        const bool z1 = (H - 1 - y1) / TILE_H == ty_top ? up_top : up_low;
        uint32_t w0[6] = { 0u, 0u, 0u, 0u, 0u, 0u }, w1[6] = { 0u, 0u, 0u, 0u, 0u, 0u };
        if (!z0) yuv_load_row<N>(a.src + ((size_t)y0 * (size_t)W + (size_t)x) * 3u, col1, w0);
        if (row1) {
            if (!z1) yuv_load_row<N>(a.src + ((size_t)y1 * (size_t)W + (size_t)x) * 3u, col1, w1);
        } else {
#pragma unroll
            for (int i = 0; i < 6; i++) w1[i] = w0[i];  // (the last row twice at an odd height)
        }
        // Y, and I444's chroma, a byte a pixel: packed four to a word
        uint32_t py[2][2] = { { 0u, 0u }, { 0u, 0u } }, pu[2][2] = { { 0u, 0u }, { 0u, 0u } }, pv[2][2] = { { 0u, 0u }, { 0u, 0u } };
        uint32_t c_lo = 0u, c_hi = 0u, d_lo = 0u;  // 4:2:0: NV12's pairs in c_lo, c_hi; I420's U in c_lo, V in d_lo
#pragma unroll
        for (int i = 0; i < N; i++) {
#pragma unroll
            for (int r = 0; r < 2; r++) {
                const uint32_t(&w)[6] = r ? w1 : w0;
                const int32_t R = yuv_byte(w, 3 * i), G = yuv_byte(w, 3 * i + 1), B = yuv_byte(w, 3 * i + 2);
                py[r][i >> 2] |= yuv_luma(k, R, G, B) << (8 * (i & 3));
                if (LAYOUT == YUV_I444) {
                    pu[r][i >> 2] |= yuv_chroma1(k.u, R, G, B) << (8 * (i & 3));
                    pv[r][i >> 2] |= yuv_chroma1(k.v, R, G, B) << (8 * (i & 3));
                }
            }
            if (LAYOUT != YUV_I444 && (i & 1)) {
                int32_t s[3];
#pragma unroll
                for (int c = 0; c < 3; c++)
                    s[c] = yuv_byte(w0, 3 * (i - 1) + c) + yuv_byte(w0, 3 * i + c) + yuv_byte(w1, 3 * (i - 1) + c) + yuv_byte(w1, 3 * i + c);
                const uint32_t U = yuv_chroma4(k.u, s[0], s[1], s[2]), V = yuv_chroma4(k.v, s[0], s[1], s[2]);
                const int j = i >> 1;  // the unit's chroma sample
                if (LAYOUT == YUV_NV12) {
                    const uint32_t pair = (U | (V << 8)) << (16 * (j & 1));
                    if (j < 2) c_lo |= pair;
                    else c_hi |= pair;
                } else {
                    c_lo |= U << (8 * j), d_lo |= V << (8 * j);
                }
            }
        }
        // stores
        uint8_t *oy0 = a.out + (size_t)y0 * (size_t)W + (size_t)x, *oy1 = a.out + (size_t)y1 * (size_t)W + (size_t)x;
        if (N == 2) {
            oy0[0] = (uint8_t)py[0][0];
            if (col1) oy0[1] = (uint8_t)(py[0][0] >> 8);
            if (row1) {
                oy1[0] = (uint8_t)py[1][0];
                if (col1) oy1[1] = (uint8_t)(py[1][0] >> 8);
            }
        } else {
            yuv_store<N>(oy0, py[0][0], py[0][1]);
            if (row1) yuv_store<N>(oy1, py[1][0], py[1][1]);
        }
        if (LAYOUT == YUV_I444) {
#pragma unroll
            for (int r = 0; r < 2; r++) {
                if (r == 1 && !row1) break;
                uint8_t *ou = (r ? oy1 : oy0) + wh, *ov = ou + wh;
                if (N == 2) {
                    ou[0] = (uint8_t)pu[r][0], ov[0] = (uint8_t)pv[r][0];
                    if (col1) ou[1] = (uint8_t)(pu[r][0] >> 8), ov[1] = (uint8_t)(pv[r][0] >> 8);
                } else {
                    yuv_store<N>(ou, pu[r][0], pu[r][1]);
                    yuv_store<N>(ov, pv[r][0], pv[r][1]);
                }
            }
        } else {
            const size_t at = (size_t)(y0 >> 1) * (size_t)cw + (size_t)(x >> 1);  // (y0 / 2 < ch, x / 2 + N / 2 <= cw)
            if (LAYOUT == YUV_NV12) {
                uint8_t *oc = a.out + wh + 2u * at;
                if (N == 2) oc[0] = (uint8_t)c_lo, oc[1] = (uint8_t)(c_lo >> 8);
                else yuv_store<N>(oc, c_lo, c_hi);
            } else {
                uint8_t *ou = a.out + wh + at, *ov = ou + (size_t)cw * (size_t)ch;
                if (N == 2) ou[0] = (uint8_t)c_lo, ov[0] = (uint8_t)d_lo;
                else yuv_store<N / 2>(ou, c_lo, 0u), yuv_store<N / 2>(ov, d_lo, 0u);
            }
        }
    }
}

// Frame statistics (tr_scene_frame_stats): the frame reduced to one record; tr_stats.h has the rule and the form of a
// partial record.  The project's one reduction, in two launches:
//   k_stats -- PERSISTENT workgroups of 1024 lanes, at most one a CU and at most one a tile (the launcher; the diagnostic
//     caps it).  A workgroup is four TEAMS of 256 lanes, four waves each; team number v = 4 * block + team of V = 4 * G
//     walks the tiles v, v + V, v + 2 V, ... of the scene's 128 x 16 tile grid (a band scene's: its band's) under k_grade's
//     permutation of a row's columns, and owns a tile the way a k_grade workgroup does: a unit is four pixels of a row,
//     twelve bytes, a lane takes two units eight rows apart.  There is no barrier inside the walk, so everything that
//     steers it need only be wave-uniform.
//       * a tile that does not meet the window is left after the comparison of its rectangle with the window's;
//       * the flags are read before any pixel.  A tile whose colour-clean flag is up holds zeros: the lane that keeps
//         the team's count adds the area of tile and window to `flat`, which goes to bin 0 of the five histograms at the
//         end; nothing is loaded.  A tile whose z-clean flag is up holds no drawn pixel: no depth is loaded.  A logically
//         cleared scene (a.cleared) is all such tiles.  The two flags are looked at independently;
//       * n_pixels is the sum of those areas whatever the path;
//       * WORDS (width % 4 == 0, fb 4-byte and z 16-byte aligned: the launcher checks): a unit's colour is three aligned
//         words, its depth one 16-byte load; otherwise guarded bytes and floats;
//       * counts go to ONE partial record in LDS (6192 bytes) by LDS atomics -- no global atomic anywhere.  Rendered
//         frames are flat: a drawn tile is mostly backdrop, a graded frame may be one colour, and 64 lanes adding to one
//         LDS word are served one after the other.  So every add is AGGREGATED over the wave (stats_add_*): the value of
//         the first lane that has one is broadcast, the lanes that hold the same value are counted by a ballot, and that
//         first lane alone adds the count; only lanes with another value add for themselves.  A wave of one colour costs
//         five adds of one lane.  Copies of the histograms per wave would not help: LDS serves one instruction of a CU at
//         a time whichever wave it comes from, and what is slow is the lanes of ONE instruction meeting on a word;
//       * a lane keeps its depth scalars (drawn, NaN, keyed min / max, box) in registers, a wave folds them by shuffles
//         at the end and its first lane adds them to the partial;
//       * behind a barrier the 1024 lanes store the partial to the workgroup's slot as 16-byte pieces, plain stores.
//   k_stats_finish -- 7 workgroups of 256 lanes, a lane a word: it sums (maxes) that word over the G slots, the last
//     workgroup turns the keyed words back (stats_publish), and every lane stores its word of the record to `out`, device
//     memory or the device address of page-locked host memory.  The launch boundary is the only ordering between the two.
// The frame, z, winner words and every flag are read only.  No inline assembly, no scratch.
constexpr int STATS_THREADS = 1024, STATS_TEAM = 256, STATS_TEAMS = STATS_THREADS / STATS_TEAM;
constexpr int STATS_FINISH_THREADS = 256;
constexpr uint32_t STATS_FINISH_BLOCKS = (STATS_WORDS + (uint32_t)STATS_FINISH_THREADS - 1u) / (uint32_t)STATS_FINISH_THREADS;
static_assert((STATS_FINISH_BLOCKS - 1u) * (uint32_t)STATS_FINISH_THREADS == SW_N_PIXELS && STATS_TAIL <= 64u,
              "the last finishing workgroup holds exactly the tail, in its first wave");

// `count` into s[bin] for every lane with act set, aggregated: the wave's first such lane adds for all that share its bin.
__device__ __forceinline__ void stats_add_bin(uint32_t *s, bool act, uint32_t bin, uint32_t lane)
{
    const unsigned long long m = __ballot(act);
    if (m == 0ull) return;  // (wave-uniform)
    const uint32_t first = (uint32_t)__ffsll((long long)m) - 1u;
    const uint32_t v0 = (uint32_t)__builtin_amdgcn_readlane((int)bin, (int)first);
    const bool same = act && bin == v0;
    const uint32_t n = (uint32_t)__popcll(__ballot(same));
    if (lane == first) atomicAdd(&s[v0], n);
    else if (act && !same) atomicAdd(&s[bin], 1u);
}

// A packed pixel (r lowest) into the five colour histograms, aggregated likewise on the whole pixel.
__device__ __forceinline__ void stats_add_colour(uint32_t *s, bool act, uint32_t px, uint32_t lane)
{
    const unsigned long long m = __ballot(act);
    if (m == 0ull) return;  // (wave-uniform)
    const uint32_t first = (uint32_t)__ffsll((long long)m) - 1u;
    const uint32_t v0 = (uint32_t)__builtin_amdgcn_readlane((int)px, (int)first);
    const bool same = act && px == v0;
    const uint32_t n = (uint32_t)__popcll(__ballot(same));
    if (lane == first || (act && !same)) {
        const uint32_t add = lane == first ? n : 1u;
        const uint32_t r = px & 0xFFu, g = (px >> 8) & 0xFFu, b = (px >> 16) & 0xFFu;
        atomicAdd(&s[0u * STATS_BINS + r], add);
        atomicAdd(&s[1u * STATS_BINS + g], add);
        atomicAdd(&s[2u * STATS_BINS + b], add);
        atomicAdd(&s[3u * STATS_BINS + stats_luma(r, g, b)], add);
        atomicAdd(&s[4u * STATS_BINS + stats_max3(r, g, b)], add);
    }
}

template <bool DEPTH, bool WORDS>
__global__ __launch_bounds__(STATS_THREADS) void k_stats(StatsArgs a)
{
    static_assert(TILE_W == 128 && TILE_H == 16 && STATS_TEAM == 256, "32 units to a row of a tile, two rounds of eight rows");
    __shared__ __align__(16) uint32_t s_rec[STATS_WORDS];
    for (uint32_t i = threadIdx.x; i < STATS_WORDS; i += STATS_THREADS) s_rec[i] = 0u;
    __syncthreads();
    const int32_t W = (int32_t)a.frame.width, H = (int32_t)a.frame.height;
    const uint32_t ntx = a.frame.ntx, n_tiles = a.frame.ntx * a.frame.nty;
    const uint32_t team = threadIdx.x / (uint32_t)STATS_TEAM, tid = threadIdx.x % (uint32_t)STATS_TEAM, lane = threadIdx.x % 64u;
    const uint32_t V = gridDim.x * (uint32_t)STATS_TEAMS;
    const StatsWindow win = a.rule.win;
    const bool cleared = a.cleared != 0u;
    uint32_t flat = 0u, n_pixels = 0u;  // (the same in every lane of a team; its lane 0 adds them)
    uint32_t n_drawn = 0u, n_nan = 0u, zmax = 0u, zminc = 0u, bx0c = 0u, by0c = 0u, bx1 = 0u, by1 = 0u;
    for (uint32_t k = blockIdx.x * (uint32_t)STATS_TEAMS + team; k < n_tiles; k += V) {
        const uint32_t tyl = k / ntx, tx = (k % ntx + 5u * tyl + 13u * (tyl * ntx / V)) % ntx;
        const uint32_t t = tyl * ntx + tx;
        const int32_t tx0 = (int32_t)tx * TILE_W, ty0 = (a.frame.ty_base + (int32_t)tyl) * TILE_H;
        // the tile's part of the window (which is cut to the frame and the band already)
        const int32_t cx0 = max(win.x0, tx0), cx1 = min(win.x1, tx0 + TILE_W), cy0 = max(win.y0, ty0), cy1 = min(win.y1, ty0 + TILE_H);
        if (cx0 >= cx1 || cy0 >= cy1) continue;
        const uint32_t area = (uint32_t)(cx1 - cx0) * (uint32_t)(cy1 - cy0);
        const bool c_clean = cleared || (a.fbclean != nullptr && a.fbclean[t] != 0u);
        const bool z_clean = !DEPTH || cleared || a.zclean[t] != 0u;
        n_pixels += area;
        if (c_clean) flat += area;
        if (c_clean && z_clean) continue;
        const int32_t x = tx0 + 4 * (int32_t)(tid % 32u);
        const int32_t y_first = ty0 + (int32_t)(tid / 32u);
        bool in_x[4];
#pragma unroll
        for (int i = 0; i < 4; i++) in_x[i] = x + i >= cx0 && x + i < cx1;
        bool row_in[2];
        uint32_t px[2][4];
        float zz[2][4];
        // both units' loads first, then the counting
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int32_t y = y_first + 8 * h;
            // (a unit of the WORDS form lies wholly inside the frame or wholly outside: width % 4 == 0)
            row_in[h] = y >= cy0 && y < cy1 && (WORDS ? x < W : true) && (in_x[0] || in_x[1] || in_x[2] || in_x[3]);
#pragma unroll
            for (int i = 0; i < 4; i++) px[h][i] = 0u, zz[h][i] = 0.0f;
            if (!row_in[h]) continue;
            if (!c_clean) {
                const uint8_t *q = a.fb + ((size_t)(H - 1 - y) * (size_t)W + (size_t)x) * 3u;
                if (WORDS) {
                    const uint32_t *qw = reinterpret_cast<const uint32_t *>(q);
                    const uint32_t w0 = qw[0], w1 = qw[1], w2 = qw[2];
                    px[h][0] = w0 & 0xFFFFFFu;
                    px[h][1] = (w0 >> 24) | ((w1 & 0xFFFFu) << 8);
                    px[h][2] = (w1 >> 16) | ((w2 & 0xFFu) << 16);
                    px[h][3] = w2 >> 8;
                } else {
#pragma unroll
                    for (int i = 0; i < 4; i++)
                        if (in_x[i]) px[h][i] = grade_pack(q[3 * i], q[3 * i + 1], q[3 * i + 2]);
                }
            }
            if (DEPTH && !z_clean) {
                const float *q = a.z + (size_t)y * (size_t)W + (size_t)x;
                if (WORDS) {
                    const float4 v = *reinterpret_cast<const float4 *>(q);
                    zz[h][0] = v.x, zz[h][1] = v.y, zz[h][2] = v.z, zz[h][3] = v.w;
                } else {
#pragma unroll
                    for (int i = 0; i < 4; i++)
                        if (in_x[i]) zz[h][i] = q[i];
                }
            }
        }
        if (!c_clean) {
#pragma unroll
            for (int h = 0; h < 2; h++)
#pragma unroll
                for (int i = 0; i < 4; i++) stats_add_colour(s_rec, row_in[h] && in_x[i], px[h][i], lane);
        }
        if (DEPTH && !z_clean) {
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const uint32_t row = (uint32_t)(H - 1 - (y_first + 8 * h));
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const uint32_t zb = f32_bits(zz[h][i]);
                    const bool drawn = row_in[h] && in_x[i] && zb != TR_F32_MIN_BITS;
                    const bool nan = stats_is_nan(zb);
                    if (drawn) {
                        const uint32_t xi = (uint32_t)(x + i);
                        n_drawn += 1u;
                        bx0c = max(bx0c, ~xi), by0c = max(by0c, ~row), bx1 = max(bx1, xi + 1u), by1 = max(by1, row + 1u);
                        if (nan) {
                            n_nan += 1u;
                        } else {
                            const uint32_t key = stats_zkey(zb);
                            zmax = max(zmax, key), zminc = max(zminc, ~key);
                        }
                    }
                    stats_add_bin(s_rec + SW_ZHIST, drawn && !nan, stats_zbin(zz[h][i], a.rule.z_lo, a.rule.z_scale), lane);
                }
            }
        }
    }
    if (tid == 0u) {
        if (n_pixels) atomicAdd(&s_rec[SW_N_PIXELS], n_pixels);
        if (flat) {
#pragma unroll
            for (uint32_t c = 0; c < STATS_HISTS; c++) atomicAdd(&s_rec[c * STATS_BINS], flat);
        }
    }
    if (DEPTH) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            n_drawn += (uint32_t)__shfl_xor((int)n_drawn, d, 64);
            n_nan += (uint32_t)__shfl_xor((int)n_nan, d, 64);
            zmax = max(zmax, (uint32_t)__shfl_xor((int)zmax, d, 64));
            zminc = max(zminc, (uint32_t)__shfl_xor((int)zminc, d, 64));
            bx0c = max(bx0c, (uint32_t)__shfl_xor((int)bx0c, d, 64));
            by0c = max(by0c, (uint32_t)__shfl_xor((int)by0c, d, 64));
            bx1 = max(bx1, (uint32_t)__shfl_xor((int)bx1, d, 64));
            by1 = max(by1, (uint32_t)__shfl_xor((int)by1, d, 64));
        }
        if (lane == 0u && n_drawn != 0u) {
            atomicAdd(&s_rec[SW_N_DRAWN], n_drawn);
            atomicAdd(&s_rec[SW_N_NAN], n_nan);
            atomicMax(&s_rec[SW_ZMAX], zmax);
            atomicMax(&s_rec[SW_ZMINC], zminc);
            atomicMax(&s_rec[SW_BX0C], bx0c);
            atomicMax(&s_rec[SW_BY0C], by0c);
            atomicMax(&s_rec[SW_BX1], bx1);
            atomicMax(&s_rec[SW_BY1], by1);
        }
    }
    __syncthreads();
    uint4 *slot = reinterpret_cast<uint4 *>(a.partials + (size_t)blockIdx.x * STATS_WORDS);
    for (uint32_t i = threadIdx.x; i < STATS_WORDS / 4u; i += STATS_THREADS) slot[i] = reinterpret_cast<const uint4 *>(s_rec)[i];
}

// partials: n_slots slots of STATS_WORDS words (k_stats' grid); depth: TR_STATS_DEPTH was given; out: STATS_WORDS words.
__global__ __launch_bounds__(STATS_FINISH_THREADS) void k_stats_finish(const uint32_t *partials, uint32_t n_slots, uint32_t depth, uint32_t *out)
{
    __shared__ uint32_t s_tail[64];
    const uint32_t i = blockIdx.x * (uint32_t)STATS_FINISH_THREADS + threadIdx.x;
    uint32_t v = 0u;
    if (i < STATS_WORDS) {
        const bool sum = i < STATS_SUMS;
        for (uint32_t g = 0; g < n_slots; g++) {
            const uint32_t p = partials[(size_t)g * STATS_WORDS + i];
            v = sum ? v + p : max(v, p);
        }
    }
    if (blockIdx.x != STATS_FINISH_BLOCKS - 1u) {
        out[i] = v;  // (i < STATS_SUMS <= STATS_WORDS here)
        return;
    }
    // words STATS_SUMS - 3 .. STATS_WORDS - 1: the counts stats_publish reads, the maxima and the reserved words
    constexpr uint32_t first = (STATS_FINISH_BLOCKS - 1u) * (uint32_t)STATS_FINISH_THREADS;
    static_assert(first == SW_N_PIXELS, "the last workgroup starts at n_pixels");
    if (threadIdx.x < STATS_TAIL) s_tail[threadIdx.x] = v;
    __syncthreads();
    if (threadIdx.x == 0u) {
        StatsTail t;
#pragma unroll
        for (uint32_t j = 0; j < STATS_TAIL; j++) t.w[j] = s_tail[j];
        stats_publish(t, depth != 0u);
#pragma unroll
        for (uint32_t j = 0; j < STATS_TAIL; j++) out[first + j] = t.w[j];
    }
}

// Dynamic textures (tr_scene_set_texture*): image `which` of a scene replaced by a w x h image of packed rgb8 rows, in
// the plain array and in the texel set together; tr_pack.h has the rule (pack_quad, shared with the host).  The grid is
// that of a frame of w x h pixels -- the image may BE one (tr_scene_set_texture_from_frame): a workgroup of 256 lanes
// covers 128 x 8 texels, half of a 128 x 16 frame tile, so the source's colour-clean flag is ONE workgroup-uniform word,
// read before any pixel: a tile whose flag is up is not loaded and packs as zeros (decode_normal(0) in the normal
// words).  A lane owns four horizontally adjacent texels:
//   * WIDE (width % 4 == 0, every base aligned: the launcher checks): their 12 source bytes are three dword loads, the
//     other image's words (word 0 of a four-word set is completed from them) one 16-byte load, the plain array's
//     words one 16-byte store; else bytes and words guarded by the width;
//   * the set's words go where packed_index puts them: one 16-byte store into an 8 x 4 block (one-word sets), the owned
//     words of 64 contiguous bytes of a 4 x 2 block (four-word sets: four word-0 stores, or words 1..3 of each texel).
// Rows of a tile count from the bottom of the frame, rows of the image from the top.  No LDS, no atomics, no scratch.
constexpr uint32_t PACK_ROWS = 8;
template <int WORDS, bool WIDE>
__global__ __launch_bounds__(256) void k_pack_texels(PackArgs a)
{
    static_assert(TILE_W == 128 && TILE_H % (int)PACK_ROWS == 0, "a workgroup is 32 quads x 8 rows of a tile");
    constexpr uint32_t PARTS = (uint32_t)TILE_H / PACK_ROWS;
    const uint32_t ntx = (a.w + (uint32_t)TILE_W - 1u) / (uint32_t)TILE_W;
    const uint32_t tile = blockIdx.x / PARTS, part = blockIdx.x % PARTS;
    const bool zeros = a.src_all_clean != 0u || (a.src_clean != nullptr && a.src_clean[tile] != 0u);  // (workgroup-uniform)
    const uint32_t cx = (tile % ntx) * (uint32_t)TILE_W + (threadIdx.x % 32u) * PACK_QUAD;
    const uint32_t y = (tile / ntx) * (uint32_t)TILE_H + part * PACK_ROWS + threadIdx.x / 32u;
    if (cx >= a.w || y >= a.h) return;
    const uint32_t cy = a.h - 1u - y;
    const uint32_t n = min(PACK_QUAD, a.w - cx);  // (WIDE: 4)
    const size_t i = (size_t)cy * a.w + cx;
    uint32_t t[PACK_QUAD] = { 0u, 0u, 0u, 0u }, o[PACK_QUAD] = { 0u, 0u, 0u, 0u };
    if (!zeros) {
        const uint8_t *p = a.src + 3u * i;
        if (WIDE) {
            // r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
            const uint32_t d0 = reinterpret_cast<const uint32_t *>(p)[0], d1 = reinterpret_cast<const uint32_t *>(p)[1],
                           d2 = reinterpret_cast<const uint32_t *>(p)[2];
            t[0] = d0 & 0xFFFFFFu;
            t[1] = (d0 >> 24) | ((d1 & 0xFFFFu) << 8);
            t[2] = (d1 >> 16) | ((d2 & 0xFFu) << 16);
            t[3] = d2 >> 8;
        } else {
#pragma unroll
            for (uint32_t k = 0; k < PACK_QUAD; k++)
                if (k < n) t[k] = pack_rgb8(p[3u * k], p[3u * k + 1u], p[3u * k + 2u]);
        }
    }
    if (a.other) {
        if (WIDE) {
            const Texel4 q = *reinterpret_cast<const Texel4 *>(a.other + i);
            o[0] = q.x, o[1] = q.y, o[2] = q.z, o[3] = q.w;
        } else {
#pragma unroll
            for (uint32_t k = 0; k < PACK_QUAD; k++)
                if (k < n) o[k] = a.other[i + k];
        }
    }
    pack_quad<WORDS, WIDE>(a, cx, cy, n, t, a.other ? o : nullptr);
}

// Morph targets (tr_scene_set_morph_weights): the posed rows of the frames of one launch.  Frame blockIdx.y blends the
// mesh's gathered rows `base` with the targets' gathered delta rows (`delta`: target k's rows start at k * n_pieces
// pieces, laid out like `base`, their uv floats unused) under its own weights into its own destination (tab.f[frame]);
// tr_morph.h has the rule.  A lane owns one 16-byte piece of a row: a row of 24 floats is positions [0..8], normals
// [9..17], uvs [18..23], so pieces 0..3 of a row are blended whole, piece 4 in its first two floats (the last normal's
// y and z) and piece 5 -- uvs -- is the mesh's own.  The weights are the same for every lane of the launch's frame:
// scalar loads, and a target of weight zero is skipped by a wave-uniform branch before its deltas are loaded.
// Per frame it reads the base rows and one set of delta rows per non-zero weight and writes the posed rows, all in
// 16-byte pieces.  The target loop is serial -- scalar load of the weight, branch, the target's load, wait -- so a small
// mesh is bound by that latency and the launch, not by memory.  No LDS, no atomics, no scratch.
__global__ __launch_bounds__(256) void k_morph(const float4 *__restrict__ base, const float4 *__restrict__ delta, uint32_t n_pieces,
                                               uint32_t n_targets, MorphTable tab)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_pieces) return;
    const MorphFrame fr = tab.f[blockIdx.y];  // (the table is in the kernel's argument segment: scalar loads)
    const constant_ptr<float> w = (constant_ptr<float>)fr.w;
    float4 *__restrict__ dst = reinterpret_cast<float4 *>(fr.dst);
    const float4 p = base[i];
    float4 v = p;
    for (uint32_t k = 0; k < n_targets; k++) {
        const float wk = w[k];
        if (wk != 0.0f) {
            const float4 d = delta[(size_t)k * n_pieces + i];
            v.x = morph_step(v.x, wk, d.x);
            v.y = morph_step(v.y, wk, d.y);
            v.z = morph_step(v.z, wk, d.z);
            v.w = morph_step(v.w, wk, d.w);
        }
    }
    const uint32_t piece = i % 6u;
    if (piece >= 4u) {
        v.z = p.z;
        v.w = p.w;
        if (piece == 5u) {
            v.x = p.x;
            v.y = p.y;
        }
    }
    dst[i] = v;
}

// Skinning (tr_scene_set_bone_palette): the skinned rows of the frames of one launch.  Frame blockIdx.y skins the rows
// tab.f[frame].src under its own palette into tab.f[frame].dst; tr_skin.h has the rule.  The workgroup first copies its
// frame's palette into LDS in 16-byte pieces -- n_bones * 6 of them, up to 768 for 256 lanes: a loop -- because the
// lanes then gather bones by index and the indices diverge across a wave: the gather is six ds_read_b128 per influence,
// not scalar or global loads.  One lane owns one polygon: its row (six 16-byte loads, six 16-byte stores) and its
// influence row (six 16-byte loads: 3 corners x 4 x {bone index, weight}).  src may be dst (a morph pose's rows, skinned
// in place behind k_morph): a lane reads only its own row, and all of it, before it writes it -- so neither pointer is
// __restrict__.  Floats 18..23, the uvs, pass through.  Every index into the row, the influences and a bone's entry is
// a compile-time constant (the loops are unrolled): nothing goes to scratch.  No atomics.  
struct LdsPalette {
    const float4 *pal;
    __device__ __forceinline__ void operator()(uint32_t b, float *e) const
    {
#pragma unroll
        for (int i = 0; i < INST_XFORM_FLOATS / 4; i++) {
            const float4 q = pal[(INST_XFORM_FLOATS / 4) * b + i];
            e[4 * i] = q.x;
            e[4 * i + 1] = q.y;
            e[4 * i + 2] = q.z;
            e[4 * i + 3] = q.w;
        }
    }
};

__global__ __launch_bounds__(256) void k_skin(const uint4 *__restrict__ infl, uint32_t n_rows, uint32_t n_bones, SkinTable tab)
{
    __shared__ float4 pal[SKIN_MAX_BONES * (INST_XFORM_FLOATS / 4)];
    const SkinFrame fr = tab.f[blockIdx.y];  // (the table is in the kernel's argument segment: scalar loads)
    const float4 *gpal = reinterpret_cast<const float4 *>(fr.pal);
    const uint32_t n_pieces = n_bones * (uint32_t)(INST_XFORM_FLOATS / 4);  // (n_bones <= SKIN_MAX_BONES: launch_skin)
    for (uint32_t i = threadIdx.x; i < n_pieces; i += 256u) pal[i] = gpal[i];
    __syncthreads();
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n_rows) return;
    const float4 *src = reinterpret_cast<const float4 *>(fr.src) + (size_t)(TRI_FLOATS / 4) * t;
    float4 *dst = reinterpret_cast<float4 *>(fr.dst) + (size_t)(TRI_FLOATS / 4) * t;
    const uint4 *in = infl + (size_t)(SKIN_ROW_WORDS / 4) * t;
    float m[TRI_FLOATS];
    uint32_t bone[3 * SKIN_INFLUENCES];
    float weight[3 * SKIN_INFLUENCES];
#pragma unroll
    for (int i = 0; i < TRI_FLOATS / 4; i++) {
        const float4 q = src[i];
        m[4 * i] = q.x;
        m[4 * i + 1] = q.y;
        m[4 * i + 2] = q.z;
        m[4 * i + 3] = q.w;
    }
#pragma unroll
    for (int i = 0; i < SKIN_ROW_WORDS / 4; i++) {
        const uint4 q = in[i];
        bone[2 * i] = q.x;
        weight[2 * i] = __uint_as_float(q.y);
        bone[2 * i + 1] = q.z;
        weight[2 * i + 1] = __uint_as_float(q.w);
    }
    const LdsPalette entry = { pal };
#pragma unroll
    for (int c = 0; c < 3; c++)
        skin_corner(entry, bone + SKIN_INFLUENCES * c, weight + SKIN_INFLUENCES * c, m + 3 * c, m + 9 + 3 * c);
#pragma unroll
    for (int i = 0; i < TRI_FLOATS / 4; i++) dst[i] = make_float4(m[4 * i], m[4 * i + 1], m[4 * i + 2], m[4 * i + 3]);
}

// tr_selftest_device_math: the device forms of the casts and of the shared-reciprocal division,
// applied to caller-chosen operands so the host can compare them with its own.
__global__ __launch_bounds__(256) void k_selftest(const float *x, const float *d, uint32_t n, uint32_t *out_u32,
                                                  int32_t *out_i32, uint32_t *out_u8, float *out_div,
                                                  float *out_div_ref)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out_u32[i] = f32_to_u32(x[i]);
    out_i32[i] = f32_to_i32(x[i]);
    out_u8[i] = f32_to_u8(x[i]);
    out_div[i] = div_by(x[i], recip_of(d[i]));
    out_div_ref[i] = x[i] / d[i];
}

// tr_selftest_shadow_fetch: the DEVICE form of shadow_fetch (tr_shaders.h) on caller-chosen coordinates, once
// through the fast-clear flags on a buffer whose flagged tiles hold stale values, once as a plain lookup in the
// materialised buffer: value bits and error bits of both, for the host to compare.
__global__ __launch_bounds__(256) void k_selftest_shadow(const float *plain, const float *stale, const uint32_t *sclean,
                                                         uint32_t W, uint32_t H, const float *x, const float *y, uint32_t n,
                                                         uint32_t *out_plain, uint32_t *out_flagged, uint32_t *err_plain,
                                                         uint32_t *err_flagged)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t e0 = 0u, e1 = 0u;
    const float a = shadow_fetch(plain, nullptr, W, H, make3(x[i], y[i], 0.0f), e0);
    const float b = shadow_fetch(stale, sclean, W, H, make3(x[i], y[i], 0.0f), e1);
    out_plain[i] = __float_as_uint(a);
    out_flagged[i] = __float_as_uint(b);
    err_plain[i] = e0;
    err_flagged[i] = e1;
}

// tr_selftest_device_unary: rcp2 / sqrt2 (tr_pk.h) against the compiler's correctly rounded
// 1.0f / x and sqrtf for every f32 whose bits lie in [first, first + count).
__global__ __launch_bounds__(256) void k_selftest_unary(int which, uint32_t first, uint64_t count,
                                                        unsigned long long *n_bad, uint32_t *bad_bits)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) {
        const float x = __uint_as_float(first + (uint32_t)i);
        float got, want;
        if (which == 2) {
            // pack_u8 (v_cvt_pk_u8_f32) against the cast it replaces, for x and -x, into every byte of a word
            const uint32_t into = 0xA5C3E17Bu, b = (uint32_t)(i & 3u);
            const uint32_t g0 = pack_u8(x, b, into), w0 = (into & ~(0xFFu << (8u * b))) | (f32_to_u8(x) << (8u * b));
            const uint32_t g1 = pack_u8(-x, b, into), w1 = (into & ~(0xFFu << (8u * b))) | (f32_to_u8(-x) << (8u * b));
            got = __uint_as_float(g0 ^ (g1 << 1) ^ (g1 >> 31));
            want = __uint_as_float(w0 ^ (w1 << 1) ^ (w1 >> 31));
            if (g0 != w0 || g1 != w1) {
                const unsigned long long k = atomicAdd(n_bad, 1ull);
                if (k < 16ull) bad_bits[k] = __float_as_uint(x);
            }
            continue;
        }
        if (which == 0) {
            got = rcp2(mk2(x, -x)).x;
            want = 1.0f / x;
            if (__float_as_uint(rcp2(mk2(x, -x)).y) != __float_as_uint(-1.0f / x)) got = __uint_as_float(~__float_as_uint(want));
        } else {
            got = sqrt2(mk2(x, x)).y;
            want = sqrtf(x);
        }
        if (__float_as_uint(got) != __float_as_uint(want)) {
            const unsigned long long k = atomicAdd(n_bad, 1ull);
            if (k < 16ull) bad_bits[k] = __float_as_uint(x);
        }
    }
}

// -----------------------------------------------------------------------------------------
// Peer exchange flags (tr_exchange.cpp): generation counters in uncached memory, possibly another
// GPU's.  Stores and loads are system scope; a waiter sleeps between polls and gives up after
// `timeout_ticks` of the 100 MHz wall clock (ten seconds unless the host says otherwise), raising the
// error word instead of hanging the queue.
// -----------------------------------------------------------------------------------------
// (`unless`: the exchange's error word -- after a wait on this queue has timed out, what was to be announced may
// not have happened: the peer is not told)
__global__ __launch_bounds__(64) void k_flag_store(uint32_t *flag, uint32_t value, const uint32_t *unless)
{
    if (threadIdx.x == 0u) {
        if (unless && __hip_atomic_load(unless, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0u) return;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
        __hip_atomic_store(flag, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// one launch tells every peer: lane p stores into peer p's block
__global__ __launch_bounds__(64) void k_flags_store_all(uint32_t *const *flags, uint32_t n, uint32_t skip, uint32_t value)
{
    if (threadIdx.x < n && threadIdx.x != skip) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
        __hip_atomic_store(flags[threadIdx.x], value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

__device__ __forceinline__ void spin_until_at_least(uint32_t *flag, uint32_t value, uint32_t *error, uint64_t timeout_ticks)
{
    const uint64_t t0 = wall_clock64();
    // generations are compared as a signed distance so that the counter may wrap
    while ((int32_t)(__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) - value) < 0) {
        __builtin_amdgcn_s_sleep(32);
        if (wall_clock64() - t0 > timeout_ticks) {
            __hip_atomic_store(error, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            break;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
}

__global__ __launch_bounds__(64) void k_flag_wait(uint32_t *flag, uint32_t value, uint32_t *error, uint64_t timeout_ticks)
{
    if (threadIdx.x == 0u) spin_until_at_least(flag, value, error, timeout_ticks);
}

__global__ __launch_bounds__(64) void k_flags_wait_all(uint32_t *const *flags, uint32_t n, uint32_t skip, uint32_t value,
                                                       uint32_t *error, uint64_t timeout_ticks)
{
    if (threadIdx.x < n && threadIdx.x != skip) spin_until_at_least(flags[threadIdx.x], value, error, timeout_ticks);
}

}  // namespace

int launch_flag_store_unless(uint32_t *flag, uint32_t value, const uint32_t *unless, hipStream_t st)
{
    hipLaunchKernelGGL(k_flag_store, dim3(1), dim3(64), 0, st, flag, value, unless);
    hipError_t e_ = hipGetLastError();
    return e_ == hipSuccess ? 0 : (int)e_;
}

int launch_flag_store(uint32_t *flag, uint32_t value, hipStream_t st) { return launch_flag_store_unless(flag, value, nullptr, st); }

int launch_flags_store_all(uint32_t *const *flags, uint32_t n, uint32_t skip, uint32_t value, hipStream_t st)
{
    if (n > 64u) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_flags_store_all, dim3(1), dim3(64), 0, st, flags, n, skip, value);
    hipError_t e_ = hipGetLastError();
    return e_ == hipSuccess ? 0 : (int)e_;
}

int launch_flag_wait(uint32_t *flag, uint32_t value, uint32_t *error, uint64_t timeout_ticks, hipStream_t st)
{
    hipLaunchKernelGGL(k_flag_wait, dim3(1), dim3(64), 0, st, flag, value, error, timeout_ticks);
    hipError_t e_ = hipGetLastError();
    return e_ == hipSuccess ? 0 : (int)e_;
}

int launch_flags_wait_all(uint32_t *const *flags, uint32_t n, uint32_t skip, uint32_t value, uint32_t *error,
                          uint64_t timeout_ticks, hipStream_t st)
{
    if (n > 64u) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_flags_wait_all, dim3(1), dim3(64), 0, st, flags, n, skip, value, error, timeout_ticks);
    hipError_t e_ = hipGetLastError();
    return e_ == hipSuccess ? 0 : (int)e_;
}

int launch_selftest_unary(int which, uint32_t first, uint64_t count, unsigned long long *n_bad, uint32_t *bad_bits,
                          hipStream_t st)
{
    if (count == 0) return 0;
    hipLaunchKernelGGL(k_selftest_unary, dim3(4096), dim3(256), 0, st, which, first, count, n_bad, bad_bits);
    hipError_t e_ = hipGetLastError();
    return e_ == hipSuccess ? 0 : (int)e_;
}

// -----------------------------------------------------------------------------------------
// Launchers
// -----------------------------------------------------------------------------------------

#define TR_LAUNCH_CHECK()                    \
    do {                                     \
        hipError_t e_ = hipGetLastError();   \
        if (e_ != hipSuccess) return (int)e_; \
    } while (0)

int rec_pieces_for_vs(int vs) { return vs == VS_DARBOUX ? REC_PIECES_LARGE : REC_PIECES_SMALL; }

// Polygons per wave of the chain's kernels: all 64 lanes beside a running tile kernel (throughput: the fewer waves, the
// less it is disturbed); when the caller's tile kernel WAITS for the chain (`hurry`, see launch_setup) and the mesh is
// small, 8 -- the wave with the most (polygon, tile) pairs is the critical path
static uint32_t chain_polys(uint32_t n_tri, uint32_t frames, bool hurry)
{
    uint32_t polys = BIN_POLYS;
    if (hurry && (uint64_t)((n_tri + polys - 1u) / polys) * frames < 2048u) polys = 8u;
    return polys;
}
int rec_pieces_for_fs(int fs) { return fs == FS_DARBOUX ? REC_PIECES_LARGE : REC_PIECES_SMALL; }

int launch_setup(int vs, const SetupArgs &a, const SetupArgs *group, uint32_t n_frames, bool xform, bool hurry, hipStream_t st,
                 hipEvent_t start, hipEvent_t done)
{
    if (!group && xform != (a.mesh.inst_xform != 0u)) return (int)hipErrorInvalidValue;
    if ((int)a.rec_pieces != rec_pieces_for_vs(vs)) return (int)hipErrorInvalidValue;
    if (group && (n_frames == 0 || n_frames > 65535u)) return (int)hipErrorInvalidValue;
    // (an empty mesh: the first workgroup still zeroes the pass's list words)
    // (`hurry`: nothing else is on the GPU and the caller's tile kernel waits for this chain -- a lone frame, or the
    // first group after a synchronisation: single waves, spread over four times as many compute units.  A per-frame
    // launch always: its chain is as long as the tile kernel it has to hide behind -- the throughput shapes made the
    // unfused per-frame loop 65 us per frame at 4096^2 where these give 38)
    hurry = hurry || !group;
    // polygons per wave: as k_bin (launch_bin), so that a wave of k_bin finds the boxes a wave of k_setup counted
    const uint32_t polys = chain_polys(a.mesh.n_tri, group ? n_frames : 1u, hurry);
    const uint32_t per_group = hurry ? 1u : CHAIN_WAVES, waves = (a.mesh.n_tri + polys - 1u) / polys;
    const dim3 grid(a.mesh.n_tri ? (waves + per_group - 1u) / per_group : 1u, group ? n_frames : 1u), block(64u * per_group);
#define TR_SETUP_CASE(V)                                                                   \
    case V:                                                                                \
        if (group && xform)                                                                \
            hipExtLaunchKernelGGL((k_setup_group<V, true>), grid, block, 0, st, start, done, 0, group, polys); \
        else if (group)                                                                    \
            hipExtLaunchKernelGGL((k_setup_group<V, false>), grid, block, 0, st, start, done, 0, group, polys); \
        else if (xform)                                                                    \
            hipExtLaunchKernelGGL((k_setup<V, true>), grid, block, 0, st, start, done, 0, a, polys); \
        else                                                                               \
            hipExtLaunchKernelGGL((k_setup<V, false>), grid, block, 0, st, start, done, 0, a, polys); \
        break;
    switch (vs) {
    TR_SETUP_CASE(VS_DEFAULT)
    TR_SETUP_CASE(VS_PHONG)
    TR_SETUP_CASE(VS_PLAIN)
    TR_SETUP_CASE(VS_DARBOUX)
    TR_SETUP_CASE(VS_DEPTH)
    default: return (int)hipErrorInvalidValue;
    }
#undef TR_SETUP_CASE
    TR_LAUNCH_CHECK();
    return 0;
}

int launch_bin(const SetupArgs &a, const SetupArgs *group, uint32_t n_frames, bool hurry, hipStream_t st, hipEvent_t start,
               hipEvent_t done)
{
    if (a.mesh.n_tri == 0) return 0;
    if (group && (n_frames == 0 || n_frames > 65535u)) return (int)hipErrorInvalidValue;
    // polygons per wave: all 64 lanes beside a running tile kernel (throughput: the fewer waves, the less it is
    // disturbed); when the caller's tile kernel WAITS for this chain (`hurry`, see launch_setup) and the mesh is
    // small, 8 -- the wave with the most (polygon, tile) pairs is the critical path (628 waves for 5 022 polygons:
    // 13 us instead of 39)
    hurry = hurry || !group;  // (see launch_setup)
    const uint32_t polys = chain_polys(a.mesh.n_tri, group ? n_frames : 1u, hurry);
    const uint32_t lds = 0u, waves = (a.mesh.n_tri + polys - 1u) / polys;
    const uint32_t per_group = hurry ? 1u : CHAIN_WAVES;
    const dim3 grid((waves + per_group - 1u) / per_group, group ? n_frames : 1u), block(64u * per_group);
    if (a.rec_pieces == (uint32_t)REC_PIECES_LARGE) {
        if (group)
            hipExtLaunchKernelGGL(k_bin_group<REC_PIECES_LARGE>, grid, block, lds, st, start, done, 0, group, polys);
        else
            hipExtLaunchKernelGGL(k_bin<REC_PIECES_LARGE>, grid, block, lds, st, start, done, 0, a, polys);
    } else if (a.rec_pieces == (uint32_t)REC_PIECES_SMALL) {
        if (group)
            hipExtLaunchKernelGGL(k_bin_group<REC_PIECES_SMALL>, grid, block, lds, st, start, done, 0, group, polys);
        else
            hipExtLaunchKernelGGL(k_bin<REC_PIECES_SMALL>, grid, block, lds, st, start, done, 0, a, polys);
    } else {
        return (int)hipErrorInvalidValue;
    }
    TR_LAUNCH_CHECK();
    return 0;
}

int launch_lit(int fs, const SetupArgs &a, const SetupArgs *group, uint32_t n_frames, hipStream_t st, hipEvent_t start, hipEvent_t done)
{
    if (!a.lit || !a.texel_set || a.tex_w == 0 || a.tex_h == 0) return (int)hipErrorInvalidValue;
    if (group && (n_frames == 0 || n_frames > 65535u)) return (int)hipErrorInvalidValue;
    const uint32_t rows = (a.tex_h + 1u) / 2u;
    const uint64_t texels = (uint64_t)a.set_bpr * rows * 8u;
    const dim3 grid((uint32_t)((texels / 2u + 255u) / 256u), group ? n_frames : 1u), block(256);  // (two texels per thread)
    if (fs == FS_SPECULAR) {
        if (group) hipExtLaunchKernelGGL(k_lit_group<FS_SPECULAR>, grid, block, 0, st, start, done, 0, group);
        else hipExtLaunchKernelGGL(k_lit<FS_SPECULAR>, grid, block, 0, st, start, done, 0, a);
    } else if (fs == FS_NORMAL_MAP) {
        if (group) hipExtLaunchKernelGGL(k_lit_group<FS_NORMAL_MAP>, grid, block, 0, st, start, done, 0, group);
        else hipExtLaunchKernelGGL(k_lit<FS_NORMAL_MAP>, grid, block, 0, st, start, done, 0, a);
    } else {
        return (int)hipErrorInvalidValue;
    }
    TR_LAUNCH_CHECK();
    return 0;
}

int launch_order(const TileArgs &one, uint32_t n_tiles, const TileArgs *group, uint32_t n_frames, hipStream_t st, hipEvent_t start,
                 hipEvent_t done)
{
    if (n_tiles == 0) return 0;
    if (group && (n_frames == 0 || n_frames > 65535u)) return (int)hipErrorInvalidValue;
    const dim3 grid((n_tiles + ORDER_THREADS - 1u) / ORDER_THREADS, group ? n_frames : 1u), block(ORDER_THREADS);
    uint32_t bits = 1;
    while ((1u << bits) < n_tiles) bits++;
    hipExtLaunchKernelGGL(k_order, grid, block, 0, st, start, done, 0, one, n_tiles, bits, group);
    TR_LAUNCH_CHECK();
    return 0;
}

// (TR_INTERIOR=0: frames of whole tiles run the general kernels like any other, as before round 6)
static bool interior_kernels()
{
    static const bool on = !getenv("TR_INTERIOR") || atoi(getenv("TR_INTERIOR")) != 0;
    return on;
}

// Is the frame made of whole tiles only -- every pixel of every tile of its grid inside the frame and the band?
// (Every frame of a fused launch has the frame and band of its scene: `a`, what the frames have in common, says it.)
static bool tile_frame_is_interior(const DevFrame &f)
{
    return f.width % (uint32_t)TILE_W == 0u && f.ntx * (uint32_t)TILE_W == f.width &&
           (int64_t)f.band_y0 == (int64_t)f.ty_base * TILE_H && (int64_t)f.band_y1 == ((int64_t)f.ty_base + (int64_t)f.nty) * TILE_H &&
           f.band_y1 >= 0 && (uint32_t)f.band_y1 <= f.height;
}

// The kernels that exist in the interior form (k_tile, INTERIOR): the fused four-wave column kernels of the light closures
template <int F, int WAVES, bool SHARED>
constexpr bool TILE_HAS_INTERIOR = WAVES == 4 && !SHARED &&
                                   (F == FS_DEFAULT || F == FS_PHONG || F == FS_LIT || F == FS_DEPTH || F == FS_SHADOW2);

bool tile_launch_is_interior(int fs, const TileArgs &a, int tile_waves, int shared, uint32_t n_polygons, bool fused)
{
    if (n_polygons > SHARED_MAX_POLYGONS) shared = 0;  // (launch_tile)
    const bool has = fs == FS_DEFAULT || fs == FS_PHONG || fs == FS_LIT || fs == FS_DEPTH || fs == FS_SHADOW2;
    return fused && has && tile_waves == 4 && !shared && interior_kernels() && tile_frame_is_interior(a.frame);
}

template <int WAVES, bool SHARED>
static int launch_tile_waves(int fs, const TileArgs &a, uint32_t n_tiles, const TileArgs *group, uint32_t n_frames,
                             hipStream_t st, hipEvent_t start, hipEvent_t done, bool fused_single)
{
    // fused_single: ONE frame that starts from cleared targets and has no winner tap runs the fused launches' kernels
    // (compiled for exactly that: no accumulate paths, no tap, eight workgroups per CU, depth left on the chip when
    // a.store says so) with its arguments by value: no table (`group` null), one frame.
    const bool fused = group != nullptr || fused_single;
    if (fused_single && !group) n_frames = 1u;
    // (n_tiles here: the workgroups per frame -- the frame's tiles, or the work units a host that knows the lists'
    // lengths asks for, plan::work_units)
    const dim3 grid(n_tiles * (fused ? n_frames : 1u)), block(64 * WAVES);
    // (a fused launch whose frames leave their depth on the chip: `a` -- what the group's frames have in common -- says so)
    const bool transient = fused && fs != FS_DEPTH && a.store == TR_STORE_COLOR;
    // (a frame of whole tiles: the same kernels without their per-pixel frame and band tests)
    const bool interior = tile_launch_is_interior(fs, a, WAVES, SHARED ? 1 : 0, 0u, fused);
#define TR_TILE_CASE(F)                                                                                                  \
    case F:                                                                                                              \
        if constexpr (TILE_HAS_INTERIOR<F, WAVES, SHARED>) {                                                             \
            if (interior) {                                                                                              \
                if (transient)                                                                                           \
                    hipExtLaunchKernelGGL((k_tile<F, WAVES, SHARED, (F == FS_DEPTH ? 1 : 2), true>), grid, block, 0, st, start, done, 0, a, group, n_frames); \
                else                                                                                                     \
                    hipExtLaunchKernelGGL((k_tile<F, WAVES, SHARED, 1, true>), grid, block, 0, st, start, done, 0, a, group, n_frames); \
                break;                                                                                                   \
            }                                                                                                            \
        }                                                                                                                \
        if (transient)                                                                                                   \
            hipExtLaunchKernelGGL((k_tile<F, WAVES, SHARED, (F == FS_DEPTH ? 1 : 2)>), grid, block, 0, st, start, done, 0, a, group, n_frames); \
        else if (fused)                                                                                                  \
            hipExtLaunchKernelGGL((k_tile<F, WAVES, SHARED, 1>), grid, block, 0, st, start, done, 0, a, group, n_frames); \
        else                                                                                                             \
            hipExtLaunchKernelGGL((k_tile<F, WAVES, SHARED, 0>), grid, block, 0, st, start, done, 0, a, nullptr, 0u); \
        break;
    switch (fs) {
    TR_TILE_CASE(FS_DEFAULT)
    TR_TILE_CASE(FS_PHONG)
    TR_TILE_CASE(FS_NORMAL_MAP)
    TR_TILE_CASE(FS_SPECULAR)
    TR_TILE_CASE(FS_DARBOUX)
    TR_TILE_CASE(FS_SHADOW2)
    TR_TILE_CASE(FS_OCCLUSION2)
    TR_TILE_CASE(FS_DEPTH)
    TR_TILE_CASE(FS_LIT)
    default: return (int)hipErrorInvalidValue;
    }
#undef TR_TILE_CASE
    TR_LAUNCH_CHECK();
    return 0;
}

int launch_tile(int fs, const TileArgs &a, int tile_waves, int shared, uint32_t n_polygons, const TileArgs *group,
                uint32_t n_frames, hipStream_t st, hipEvent_t start, hipEvent_t done, uint32_t units_per_frame, bool fused_single)
{
    uint32_t n_tiles = a.frame.ntx * a.frame.nty;
    if (n_tiles == 0) return 0;
    // workgroups per frame: one per tile always suffices (units <= tiles); fewer when the caller knows the lists' lengths
    if (units_per_frame != 0u && units_per_frame < n_tiles) n_tiles = units_per_frame;
    if ((int)a.rec_pieces != rec_pieces_for_fs(fs)) return (int)hipErrorInvalidValue;
    if (group && (n_frames == 0 || (uint64_t)n_tiles * n_frames > 0x7FFFFFFFull)) return (int)hipErrorInvalidValue;
    if (fused_single && (group || a.fresh == 0u || a.winner)) return (int)hipErrorInvalidValue;  // (what those kernels are compiled for)
    // the shared keys pack polygon id and bin slot into 32 bits: beyond their fields, resolve by columns
    if (n_polygons > SHARED_MAX_POLYGONS) shared = 0;  // (a tile with more records than the slot field holds resolves by columns: k_tile)
    if (shared) {
        if (tile_waves == 16) return launch_tile_waves<16, true>(fs, a, n_tiles, group, n_frames, st, start, done, fused_single);
        if (tile_waves == 8) return launch_tile_waves<8, true>(fs, a, n_tiles, group, n_frames, st, start, done, fused_single);
        if (tile_waves == 4) return launch_tile_waves<4, true>(fs, a, n_tiles, group, n_frames, st, start, done, fused_single);
    } else {
        if (tile_waves == 16) return launch_tile_waves<16, false>(fs, a, n_tiles, group, n_frames, st, start, done, fused_single);
        if (tile_waves == 8) return launch_tile_waves<8, false>(fs, a, n_tiles, group, n_frames, st, start, done, fused_single);
        if (tile_waves == 4) return launch_tile_waves<4, false>(fs, a, n_tiles, group, n_frames, st, start, done, fused_single);
    }
    return (int)hipErrorInvalidValue;
}

int launch_materialize_depth(float *zbuf, uint32_t *zclean, const DevFrame &frame, hipStream_t st)
{
    const uint32_t n_tiles = frame.ntx * frame.nty;
    if (n_tiles == 0) return 0;
    hipLaunchKernelGGL(k_materialize_depth, dim3(n_tiles), dim3(256), 0, st, zbuf, zclean, frame);
    TR_LAUNCH_CHECK();
    return 0;
}

int launch_selftest(const float *x, const float *d, uint32_t n, uint32_t *out_u32, int32_t *out_i32,
                    uint32_t *out_u8, float *out_div, float *out_div_ref, hipStream_t st)
{
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_selftest, dim3((n + 255u) / 256u), dim3(256), 0, st, x, d, n, out_u32, out_i32, out_u8,
                       out_div, out_div_ref);
    TR_LAUNCH_CHECK();
    return 0;
}

int launch_read_back(const uint8_t *fb, uint8_t *host, const uint32_t *fb_clean, uint32_t *host_clean, const DevFrame &frame,
                     hipStream_t st)
{
    const uint32_t n_tiles = frame.ntx * frame.nty;
    if (n_tiles == 0) return 0;
    if (frame.width % 16u) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_read_back, dim3(n_tiles), dim3(256), 0, st, fb, host, fb_clean, host_clean, frame);
    TR_LAUNCH_CHECK();
    return 0;
}

int launch_push_tiles(const uint8_t *fb, uint8_t *peer, const uint32_t *fb_clean, uint32_t *remote_clean, const DevFrame &frame,
                      const uint32_t *poisoned, unsigned long long *bytes, hipStream_t st)
{
    const uint32_t n_tiles = frame.ntx * frame.nty;
    if (n_tiles == 0) return 0;
    if (frame.width % 16u) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_push_tiles, dim3(n_tiles), dim3(256), 0, st, fb, peer, fb_clean, remote_clean, frame, poisoned, bytes);
    TR_LAUNCH_CHECK();
    return 0;
}

template <int F>
static int launch_resolve_f(const uint8_t *fb, uint8_t *out, const uint32_t *fb_clean, const DevFrame &frame, bool wide,
                            hipStream_t st)
{
    const uint32_t n_tiles = frame.ntx * frame.nty, per_block = 64u / (8u * (uint32_t)(TILE_H / F));
    const dim3 grid((n_tiles + per_block - 1u) / per_block);
    if (wide)
        hipLaunchKernelGGL((k_resolve<F, true>), grid, dim3(64), 0, st, fb, out, fb_clean, frame);
    else
        hipLaunchKernelGGL((k_resolve<F, false>), grid, dim3(64), 0, st, fb, out, fb_clean, frame);
    TR_LAUNCH_CHECK();
    return 0;
}

int launch_resolve(const uint8_t *fb, uint8_t *out, const uint32_t *fb_clean, const DevFrame &frame, uint32_t factor,
                   hipStream_t st)
{
    if (frame.ntx * frame.nty == 0) return 0;
    if ((factor != 2u && factor != 4u && factor != 8u) || frame.width % factor || frame.height % factor ||
        frame.band_y0 % (int32_t)factor || frame.band_y1 % (int32_t)factor)
        return (int)hipErrorInvalidValue;
    // the wide path: source rows in 16-byte pieces, a share's 48 / factor output bytes in three aligned stores
    const uintptr_t store = 16u / factor, out_row = (uintptr_t)(frame.width / factor) * 3u;
    const bool wide = frame.width % 16u == 0u && (uintptr_t)fb % 16u == 0u && (uintptr_t)out % store == 0u && out_row % store == 0u;
    if (factor == 2u) return launch_resolve_f<2>(fb, out, fb_clean, frame, wide, st);
    if (factor == 4u) return launch_resolve_f<4>(fb, out, fb_clean, frame, wide, st);
    return launch_resolve_f<8>(fb, out, fb_clean, frame, wide, st);
}

int launch_composite(const CompositeArgs &a, hipStream_t st)
{
    const uint32_t n_tiles = a.frame.ntx * a.frame.nty;
    if (n_tiles == 0) return 0;
    if (!a.dst_z || !a.dst_fb || !a.dst_zclean || !a.dst_fbclean || !a.src_z || !a.src_fb || !a.src_zclean ||
        (a.dst_winner && !a.src_winner))
        return (int)hipErrorInvalidValue;
    // the wide path: every share is whole 16-byte pieces of z, colour and winner words
    const uintptr_t all = (uintptr_t)a.dst_z | (uintptr_t)a.dst_fb | (uintptr_t)a.dst_winner | (uintptr_t)a.src_z |
                          (uintptr_t)a.src_fb | (uintptr_t)(a.dst_winner ? a.src_winner : nullptr);
    const bool wide = a.frame.width % 16u == 0u && all % 16u == 0u;
    if (wide)
        hipLaunchKernelGGL((k_composite<true>), dim3(n_tiles), dim3(8 * TILE_H), 0, st, a);
    else
        hipLaunchKernelGGL((k_composite<false>), dim3(n_tiles), dim3(8 * TILE_H), 0, st, a);
    TR_LAUNCH_CHECK();
    return 0;
}

int launch_shadow_merge(const ShadowMergeArgs &a, hipStream_t st)
{
    const uint32_t n_tiles = a.frame.ntx * a.frame.nty;
    if (n_tiles == 0) return 0;
    if (!a.dst || !a.dst_clean || !a.src || !a.src_clean) return (int)hipErrorInvalidValue;
    // the wide path: every piece is one aligned 16-byte word of each buffer
    const bool wide = a.frame.width % 4u == 0u && ((uintptr_t)a.dst | (uintptr_t)a.src) % 16u == 0u;
    if (wide)
        hipLaunchKernelGGL((k_shadow_merge<true>), dim3(n_tiles), dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL((k_shadow_merge<false>), dim3(n_tiles), dim3(256), 0, st, a);
    TR_LAUNCH_CHECK();
    return 0;
}

int launch_ao(const AoArgs &a, hipStream_t st)
{
    const uint32_t n_tiles = a.frame.ntx * a.frame.nty;
    if (n_tiles == 0) return 0;
    if (!a.z || !a.zclean || !a.fb || !a.fbclean) return (int)hipErrorInvalidValue;
    // the whole frame's tile grid (a band's halo would lie on another rank), samples inside the staged halo
    if (a.frame.ty_base != 0 || a.frame.band_y0 != 0 || a.frame.band_y1 != (int32_t)a.frame.height) return (int)hipErrorInvalidValue;
    if (a.radius == 0u || a.radius > (uint32_t)AO_MAX_RADIUS || a.n_taps > (uint32_t)(AO_MAX_RINGS * AO_RING))
        return (int)hipErrorInvalidValue;
    for (uint32_t i = 0; i < a.n_taps; i++)
        if (abs((int)a.taps.d[i][0]) > (int)a.radius || abs((int)a.taps.d[i][1]) > (int)a.radius) return (int)hipErrorInvalidValue;
    // the wide path: every share is whole 16-byte pieces of z and colour
    const bool wide = a.frame.width % 16u == 0u && ((uintptr_t)a.z | (uintptr_t)a.fb) % 16u == 0u;
    if (wide)
        hipLaunchKernelGGL((k_ao<true>), dim3(n_tiles), dim3(AO_THREADS), 0, st, a);
    else
        hipLaunchKernelGGL((k_ao<false>), dim3(n_tiles), dim3(AO_THREADS), 0, st, a);
    TR_LAUNCH_CHECK();
    return 0;
}

int launch_dof(const DofArgs &a, hipStream_t st)
{
    const uint32_t n_tiles = a.frame.ntx * a.frame.nty;
    if (n_tiles == 0) return 0;
    if (!a.z || !a.zclean || !a.fb || !a.out) return (int)hipErrorInvalidValue;
    // the whole frame's tile grid (a band's halo would lie on another rank), taps inside the staged halo
    if (a.frame.ty_base != 0 || a.frame.band_y0 != 0 || a.frame.band_y1 != (int32_t)a.frame.height) return (int)hipErrorInvalidValue;
    if (a.rule.max_radius == 0u || a.rule.max_radius > (uint32_t)DOF_MAX_RADIUS || a.rule.background_radius > a.rule.max_radius)
        return (int)hipErrorInvalidValue;
    // `out` is never the frame that is read
    const size_t bytes = (size_t)a.frame.width * a.frame.height * 3u;
    if ((const uint8_t *)a.out < a.fb + bytes && a.fb < (const uint8_t *)a.out + bytes) return (int)hipErrorInvalidValue;
    // the wide path: every share is whole 16-byte pieces of z and colour
    const bool wide = a.frame.width % 16u == 0u && ((uintptr_t)a.z | (uintptr_t)a.fb | (uintptr_t)a.out) % 16u == 0u;
    const size_t lds = (size_t)(TILE_H + 2 * (int)a.rule.max_radius) * DOF_LDS_W * sizeof(uint2);
    if (wide)
        hipLaunchKernelGGL((k_dof<true>), dim3(n_tiles), dim3(DOF_THREADS), lds, st, a);
    else
        hipLaunchKernelGGL((k_dof<false>), dim3(n_tiles), dim3(DOF_THREADS), lds, st, a);
    TR_LAUNCH_CHECK();
    return 0;
}

int launch_bloom(const BloomArgs &a, hipStream_t st)
{
    const uint32_t n_tiles = a.frame.ntx * a.frame.nty;
    if (n_tiles == 0) return 0;
    if (!a.fb || !a.out) return (int)hipErrorInvalidValue;
    // the whole frame's tile grid (a band's halo would lie on another rank), taps inside the staged halo, sums that fit
    if (a.frame.ty_base != 0 || a.frame.band_y0 != 0 || a.frame.band_y1 != (int32_t)a.frame.height) return (int)hipErrorInvalidValue;
    if (a.rule.radius == 0u || a.rule.radius > (uint32_t)BLOOM_MAX_RADIUS || a.rule.threshold > 255u || a.rule.strength > BLOOM_MAX_STRENGTH)
        return (int)hipErrorInvalidValue;
    // `out` is never the frame that is read
    const size_t bytes = (size_t)a.frame.width * a.frame.height * 3u;
    if ((const uint8_t *)a.out < a.fb + bytes && a.fb < (const uint8_t *)a.out + bytes) return (int)hipErrorInvalidValue;
    // the wide path: every share and every staged piece is whole aligned words of colour
    const bool wide = a.frame.width % 16u == 0u && ((uintptr_t)a.fb | (uintptr_t)a.out) % 16u == 0u;
    // keyed pixels (a word each), the words {r | b << 16} and the u16 g of the horizontal sums
    const size_t lds = (size_t)(TILE_H + 2 * (int)a.rule.radius) * ((size_t)BLOOM_LDS_W * 4u + (size_t)TILE_W * 6u);
    if (wide)
        hipLaunchKernelGGL((k_bloom<true>), dim3(n_tiles), dim3(BLOOM_THREADS), lds, st, a);
    else
        hipLaunchKernelGGL((k_bloom<false>), dim3(n_tiles), dim3(BLOOM_THREADS), lds, st, a);
    TR_LAUNCH_CHECK();
    return 0;
}

// What launch_convolve, launch_rank and launch_bilateral share: the refusals of a stage that reads neighbours (ok), a.words, the store
// form (k_convolve's STORE) and the LDS of the staged rows.
struct NeighPlan {
    bool ok;
    int store;
    size_t lds;
};

template <typename Args>
static NeighPlan neigh_plan(Args &a)
{
    NeighPlan plan = { false, 0, (size_t)(TILE_H + 2 * (int)(a.rule.kh / 2u)) * CONV_LDS_W * 4u };
    if (!a.fb || !a.out) return plan;
    // the whole frame's tile grid (a band's halo would lie on another rank), taps inside the staged halo
    if (a.frame.ty_base != 0 || a.frame.band_y0 != 0 || a.frame.band_y1 != (int32_t)a.frame.height) return plan;
    // `out` is never the frame that is read
    const size_t bytes = (size_t)a.frame.width * a.frame.height * 3u;
    if ((const uint8_t *)a.out < a.fb + bytes && a.fb < (const uint8_t *)a.out + bytes) return plan;
    // staging by words: four pixels at a multiple of four are three aligned words of the frame
    a.words = a.frame.width % 4u == 0u && (uintptr_t)a.fb % 4u == 0u ? 1u : 0u;
    // the stores: every share three whole 16-byte pieces of `out`, else whole 12-byte pieces at multiples of 4, else bytes
    plan.store = a.frame.width % 16u == 0u && (uintptr_t)a.out % 16u == 0u ? 2 : a.frame.width % 4u == 0u && (uintptr_t)a.out % 4u == 0u ? 1 : 0;
    plan.ok = true;
    return plan;
}

int launch_convolve(const ConvolveArgs &a0, hipStream_t st)
{
    ConvolveArgs a = a0;
    const uint32_t n_tiles = a.frame.ntx * a.frame.nty;
    if (n_tiles == 0) return 0;
    const NeighPlan plan = neigh_plan(a);
    const bool sep = (a.rule.flags & CONVOLVE_SEPARABLE) != 0u;
    const uint32_t k_max = sep ? (uint32_t)CONVOLVE_MAX_SEPARABLE : (uint32_t)CONVOLVE_MAX_GENERAL;
    if (!plan.ok || a.rule.kw % 2u == 0u || a.rule.kh % 2u == 0u || a.rule.kw > k_max || a.rule.kh > k_max || a.rule.shift > CONVOLVE_MAX_SHIFT ||
        a.rule.edge > CONVOLVE_CLAMP || a.rule.amount > CONVOLVE_MAX_AMOUNT)
        return (int)hipErrorInvalidValue;
    int64_t col_sum = 0;
    for (uint32_t j = 0; sep && j < a.rule.kh; j++) col_sum += std::abs((int64_t)a.rule.weights[a.rule.kw + j]);
    a.rule.mul24 = sep && col_sum <= CONVOLVE_MAX_ROW ? 1 : 0;
    const size_t lds = plan.lds + (sep ? (size_t)3 * TILE_H * CONV_LDS_W * 4u : 0u);
    // [general, separable in 24 bits, separable in 32][STORE]
    static constexpr void (*kernels[3][3])(ConvolveArgs) = {
        { k_convolve<false, 0, true>, k_convolve<false, 1, true>, k_convolve<false, 2, true> },
        { k_convolve<true, 0, true>, k_convolve<true, 1, true>, k_convolve<true, 2, true> },
        { k_convolve<true, 0, false>, k_convolve<true, 1, false>, k_convolve<true, 2, false> },
    };
    hipLaunchKernelGGL(kernels[!sep ? 0 : a.rule.mul24 ? 1 : 2][plan.store], dim3(n_tiles), dim3(CONV_THREADS), lds, st, a);
    TR_LAUNCH_CHECK();
    return 0;
}

int launch_rank(const RankArgs &a0, hipStream_t st)
{
    RankArgs a = a0;
    const uint32_t n_tiles = a.frame.ntx * a.frame.nty;
    if (n_tiles == 0) return 0;
    const NeighPlan plan = neigh_plan(a);
    const RankRule &q = a.rule;
    if (!plan.ok || q.kw % 2u == 0u || q.kh % 2u == 0u || q.kw > RANK_MAX_SIDE || q.kh > RANK_MAX_SIDE || q.op > RANK_CLAMP_CENTRE || q.edge > RANK_CLAMP ||
        q.n == 0u || q.n > q.kw * q.kh || q.rank > q.rank2 || q.rank2 >= q.n)
        return (int)hipErrorInvalidValue;
    // the extremes need no selection: every rank asked for is the first or the last; bit 0 -- the minimum, bit 1 -- the maximum
    const bool extremes = (q.rank == 0u || q.rank == q.n - 1u) && (q.rank2 == 0u || q.rank2 == q.n - 1u);
    const int sel = !extremes ? 0 : ((q.rank == 0u || q.rank2 == 0u) ? 1 : 0) | ((q.rank != 0u || q.rank2 != 0u) ? 2 : 0);
    // [SEL][STORE]
    static constexpr void (*kernels[4][3])(RankArgs) = {
        { k_rank<0, 0>, k_rank<0, 1>, k_rank<0, 2> },
        { k_rank<1, 0>, k_rank<1, 1>, k_rank<1, 2> },
        { k_rank<2, 0>, k_rank<2, 1>, k_rank<2, 2> },
        { k_rank<3, 0>, k_rank<3, 1>, k_rank<3, 2> },
    };
    hipLaunchKernelGGL(kernels[sel][plan.store], dim3(n_tiles), dim3(CONV_THREADS), plan.lds, st, a);
    TR_LAUNCH_CHECK();
    return 0;
}

int launch_bilateral(const BilateralArgs &a0, hipStream_t st)
{
    BilateralArgs a = a0;
    const uint32_t n_tiles = a.frame.ntx * a.frame.nty;
    if (n_tiles == 0) return 0;
    const NeighPlan plan = neigh_plan(a);
    const BilateralRule &q = a.rule;
    const bool depth = q.guide == BILATERAL_GUIDE_DEPTH;
    if (!plan.ok || q.kw % 2u == 0u || q.kh % 2u == 0u || q.kw > BILATERAL_MAX_SIDE || q.kh > BILATERAL_MAX_SIDE || q.guide > BILATERAL_GUIDE_DEPTH ||
        q.edge > BILATERAL_CLAMP || (depth && !a.z))
        return (int)hipErrorInvalidValue;
    // the staged colour, as much again for the depth, and the range table
    const size_t lds = plan.lds * (depth ? 2u : 1u) + 256u;
    // [GUIDE][STORE]
    static constexpr void (*kernels[2][3])(BilateralArgs) = {
        { k_bilateral<0, 0>, k_bilateral<0, 1>, k_bilateral<0, 2> },
        { k_bilateral<1, 0>, k_bilateral<1, 1>, k_bilateral<1, 2> },
    };
    hipLaunchKernelGGL(kernels[depth ? 1 : 0][plan.store], dim3(n_tiles), dim3(CONV_THREADS), lds, st, a);
    TR_LAUNCH_CHECK();
    return 0;
}

int launch_grade(const GradeArgs &a, hipStream_t st, uint32_t cap, uint32_t *grid_out)
{
    *grid_out = 0u;
    const uint32_t n_tiles = a.frame.ntx * a.frame.nty;
    if (n_tiles == 0) return 0;
    if (!a.fb || !a.out || !a.lut || a.rule.n < 2u || a.rule.n > GRADE_MAX_N || (uintptr_t)a.lut % 16u != 0u) return (int)hipErrorInvalidValue;
    // `out` is the frame itself or apart from it; a flag is lowered in place only
    const size_t bytes = (size_t)a.frame.width * a.frame.height * 3u;
    if (a.out != a.fb && (const uint8_t *)a.out < a.fb + bytes && a.fb < (const uint8_t *)a.out + bytes) return (int)hipErrorInvalidValue;
    if (a.lower_clean != nullptr && (a.out != a.fb || a.lower_clean != a.fbclean || a.rule.c0 == 0u)) return (int)hipErrorInvalidValue;
    // whole words: every unit of four pixels is three aligned words of either buffer
    const bool words = a.frame.width % 4u == 0u && ((uintptr_t)a.fb | (uintptr_t)a.out) % 4u == 0u;
    const bool lds = a.rule.n <= GRADE_LDS_MAX_N;
    const size_t lds_bytes = lds ? (size_t)((a.rule.n * a.rule.n * a.rule.n + 3u) / 4u) * 16u : 0u;
    // persistent workgroups: as many as the device holds at once -- per CU what its LDS admits beside the waves' limit
    int dev = 0, cus = 0, lds_per_cu = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
        return (int)hipErrorInvalidDevice;
    if (hipDeviceGetAttribute(&lds_per_cu, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, dev) != hipSuccess || lds_per_cu < 65536)
        lds_per_cu = 65536;
    uint32_t per_cu = (uint32_t)GRADE_MAX_PER_CU;
    if (lds) per_cu = std::min<uint32_t>(per_cu, (uint32_t)((size_t)lds_per_cu / lds_bytes));
    uint32_t grid = std::min<uint32_t>((uint32_t)cus * per_cu, n_tiles);
    if (cap != 0u) grid = std::min<uint32_t>(grid, cap);  // (the diagnostic: fewer workgroups, more rounds each)
    *grid_out = grid;
    if (lds && words)
        hipLaunchKernelGGL((k_grade<true, true>), dim3(grid), dim3(GRADE_THREADS), lds_bytes, st, a);
    else if (lds)
        hipLaunchKernelGGL((k_grade<true, false>), dim3(grid), dim3(GRADE_THREADS), lds_bytes, st, a);
    else if (words)
        hipLaunchKernelGGL((k_grade<false, true>), dim3(grid), dim3(GRADE_THREADS), 0, st, a);
    else
        hipLaunchKernelGGL((k_grade<false, false>), dim3(grid), dim3(GRADE_THREADS), 0, st, a);
    TR_LAUNCH_CHECK();
    return 0;
}

int launch_ramp(const RampArgs &a, hipStream_t st, uint32_t cap, uint32_t *grid_out)
{
    *grid_out = 0u;
    const uint32_t W = a.frame.width, H = a.frame.height, n_tiles = a.frame.ntx * a.frame.nty;
    if (n_tiles == 0) return 0;
    const RampRule &q = a.rule;
    if (!a.fb || !a.out || !a.z || !a.zclean || !a.table || (uintptr_t)a.table % 16u != 0u) return (int)hipErrorInvalidValue;
    // the whole frame's tile grid (both flag sets and z are indexed by it), the rule's limits
    if (a.frame.ty_base != 0 || a.frame.band_y0 != 0 || a.frame.band_y1 != (int32_t)H) return (int)hipErrorInvalidValue;
    if (a.frame.ntx != (W + TILE_W - 1) / TILE_W || a.frame.nty != (H + TILE_H - 1) / TILE_H) return (int)hipErrorInvalidValue;
    if (q.n < 2u || q.n > RAMP_MAX_N || q.mode >= LAYER_MODES || q.opacity > 256u || (q.flags & ~RAMP_REPEAT) != 0u) return (int)hipErrorInvalidValue;
    // `out` is the frame itself or apart from it; a flag is lowered in place only
    const size_t bytes = (size_t)W * H * 3u;
    if (a.out != a.fb && (const uint8_t *)a.out < a.fb + bytes && a.fb < (const uint8_t *)a.out + bytes) return (int)hipErrorInvalidValue;
    if (a.lower != nullptr && (a.out != a.fb || a.lower != a.fbclean)) return (int)hipErrorInvalidValue;
    // whole words: every unit of four pixels is three aligned words of either buffer, its depths one 16-byte piece
    const bool words = W % 4u == 0u && ((uintptr_t)a.fb | (uintptr_t)a.out) % 4u == 0u && (uintptr_t)a.z % 16u == 0u;
    const size_t lds_bytes = (size_t)((q.n + 3u) / 4u) * 16u;
    // persistent workgroups: as many as the device holds at once (at most 8 x 4 KB of LDS a CU: the waves are the limit)
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
        return (int)hipErrorInvalidDevice;
    uint32_t grid = std::min<uint32_t>((uint32_t)cus * (uint32_t)RAMP_MAX_PER_CU, n_tiles);
    if (cap != 0u) grid = std::min<uint32_t>(grid, cap);  // (the diagnostic: fewer workgroups, more rounds each)
    *grid_out = grid;
    if (words)
        hipLaunchKernelGGL((k_ramp<true>), dim3(grid), dim3(RAMP_THREADS), lds_bytes, st, a);
    else
        hipLaunchKernelGGL((k_ramp<false>), dim3(grid), dim3(RAMP_THREADS), lds_bytes, st, a);
    TR_LAUNCH_CHECK();
    return 0;
}

static int dist_args_ok(const DistArgs &a)
{
    const uint32_t W = a.frame.width, H = a.frame.height;
    if (W == 0u || H == 0u || !a.mask || !a.h || !a.summary) return (int)hipErrorInvalidValue;
    // the whole frame's tile grid (both flag sets are indexed by it), the rule's limits
    if (a.frame.ty_base != 0 || a.frame.band_y0 != 0 || a.frame.band_y1 != (int32_t)H) return (int)hipErrorInvalidValue;
    if (a.frame.ntx != (W + TILE_W - 1) / TILE_W || a.frame.nty != (H + TILE_H - 1) / TILE_H) return (int)hipErrorInvalidValue;
    if (a.rule.seed > DIST_SEED_KEY || a.rule.threshold > 255u || a.rule.radius < 1u || a.rule.radius > DIST_MAX_RADIUS || (a.rule.flags & ~DIST_INVERT) != 0u)
        return (int)hipErrorInvalidValue;
    if ((H + DIST_ROWS - 1) / DIST_ROWS > 65535u) return (int)hipErrorInvalidValue;
    return 0;
}

static dim3 dist_grid(const DistArgs &a) { return dim3(dist_words_per_row(a.frame.width), (a.frame.height + DIST_ROWS - 1) / DIST_ROWS); }

int launch_dist_mask(const DistArgs &a, hipStream_t st)
{
    int rc = dist_args_ok(a);
    if (rc) return rc;
    if (!a.fb || (a.rule.seed == DIST_SEED_DRAWN && (!a.z || !a.zclean))) return (int)hipErrorInvalidValue;
    if (a.rule.seed == DIST_SEED_KEY)
        hipLaunchKernelGGL((k_dist_mask<true>), dist_grid(a), dim3(DIST_THREADS), 0, st, a);
    else
        hipLaunchKernelGGL((k_dist_mask<false>), dist_grid(a), dim3(DIST_THREADS), 0, st, a);
    TR_LAUNCH_CHECK();
    return 0;
}

int launch_dist_row(const DistArgs &a, hipStream_t st)
{
    int rc = dist_args_ok(a);
    if (rc) return rc;
    hipLaunchKernelGGL(k_dist_row, dist_grid(a), dim3(DIST_THREADS), 0, st, a);
    TR_LAUNCH_CHECK();
    return 0;
}

int launch_dist(const DistArgs &a, hipStream_t st)
{
    int rc = dist_args_ok(a);
    if (rc) return rc;
    if (!a.field || (uintptr_t)a.field % 2u != 0u) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_dist, dist_grid(a), dim3(DIST_THREADS), 0, st, a);
    TR_LAUNCH_CHECK();
    return 0;
}

int launch_dist_apply(const DistApplyArgs &a, hipStream_t st)
{
    const uint32_t W = a.frame.width, H = a.frame.height, n_tiles = a.frame.ntx * a.frame.nty;
    if (n_tiles == 0) return 0;
    const DistRampRule &q = a.rule;
    if (!a.fb || !a.out || !a.field || (uintptr_t)a.field % 8u != 0u || !a.table || (uintptr_t)a.table % 16u != 0u) return (int)hipErrorInvalidValue;
    if (a.frame.ty_base != 0 || a.frame.band_y0 != 0 || a.frame.band_y1 != (int32_t)H) return (int)hipErrorInvalidValue;
    if (a.frame.ntx != (W + TILE_W - 1) / TILE_W || a.frame.nty != (H + TILE_H - 1) / TILE_H) return (int)hipErrorInvalidValue;
    if (q.n < 2u || q.n > RAMP_MAX_N || q.mode >= LAYER_MODES || q.opacity > 256u || (q.flags & ~(DIST_REPEAT | DIST_KEEP_SEEDS)) != 0u || q.step < 1u ||
        q.step > DIST_MAX_STEP)
        return (int)hipErrorInvalidValue;
    // `out` is the frame itself or apart from it; a flag is lowered in place only
    const size_t bytes = (size_t)W * H * 3u;
    if (a.out != a.fb && (const uint8_t *)a.out < a.fb + bytes && a.fb < (const uint8_t *)a.out + bytes) return (int)hipErrorInvalidValue;
    if (a.lower != nullptr && (a.out != a.fb || a.lower != a.fbclean)) return (int)hipErrorInvalidValue;
    const bool words = W % 4u == 0u && ((uintptr_t)a.fb | (uintptr_t)a.out) % 4u == 0u;
    const size_t lds_bytes = (size_t)((q.n + 3u) / 4u) * 16u;
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
        return (int)hipErrorInvalidDevice;
    const uint32_t grid = std::min<uint32_t>((uint32_t)cus * (uint32_t)RAMP_MAX_PER_CU, n_tiles);
    if (words)
        hipLaunchKernelGGL((k_dist_apply<true>), dim3(grid), dim3(RAMP_THREADS), lds_bytes, st, a);
    else
        hipLaunchKernelGGL((k_dist_apply<false>), dim3(grid), dim3(RAMP_THREADS), lds_bytes, st, a);
    TR_LAUNCH_CHECK();
    return 0;
}

template <bool WORDS, int FORMAT>
static void launch_layer_form(const LayerArgs &a, bool where, hipStream_t st)
{
    const dim3 grid(a.gnx * a.gny), block(LAYER_THREADS);
    if (where)
        hipLaunchKernelGGL((k_layer<WORDS, FORMAT, true>), grid, block, 0, st, a);
    else
        hipLaunchKernelGGL((k_layer<WORDS, FORMAT, false>), grid, block, 0, st, a);
}

int launch_layer(const LayerArgs &a_in, bool from_scene, hipStream_t st)
{
    LayerArgs a = a_in;
    const uint32_t W = a.frame.width, H = a.frame.height;
    if (a.frame.ntx * a.frame.nty == 0) return 0;
    if (!a.fb || !a.out) return (int)hipErrorInvalidValue;
    // the whole frame's tile grid (the flags are indexed by it), the rule's limits
    if (a.frame.ty_base != 0 || a.frame.band_y0 != 0 || a.frame.band_y1 != (int32_t)H) return (int)hipErrorInvalidValue;
    if (a.frame.ntx != (W + TILE_W - 1) / TILE_W || a.frame.nty != (H + TILE_H - 1) / TILE_H) return (int)hipErrorInvalidValue;
    const LayerRule &q = a.rule;
    const uint32_t where_flags = q.flags & (LAYER_WHERE_DRAWN | LAYER_WHERE_UNDRAWN);
    if (q.mode >= LAYER_MODES || q.format > LAYER_RGBA8 || (q.flags & ~(LAYER_KEY | LAYER_WHERE_DRAWN | LAYER_WHERE_UNDRAWN)) != 0u ||
        where_flags == (LAYER_WHERE_DRAWN | LAYER_WHERE_UNDRAWN) || q.opacity > 256u || q.width < 1u || q.width > LAYER_MAX_SIDE ||
        q.height < 1u || q.height > LAYER_MAX_SIDE || q.stride < q.width * layer_bpp(q.format))
        return (int)hipErrorInvalidValue;
    if (from_scene && (q.format != LAYER_RGB8 || (a.src_clean && a.src_ntx != (q.width + TILE_W - 1) / TILE_W))) return (int)hipErrorInvalidValue;
    if (!from_scene && (a.src_clean || a.src_all_clean)) return (int)hipErrorInvalidValue;
    if (where_flags != 0u && (!a.z || !a.zclean)) return (int)hipErrorInvalidValue;
    if (!a.image && !a.src_all_clean) return (int)hipErrorInvalidValue;
    // `out` is the frame itself or apart from it; a flag is lowered in place only; the layer is apart from both
    const size_t bytes = (size_t)W * H * 3u;
    if (a.out != a.fb && (const uint8_t *)a.out < a.fb + bytes && a.fb < (const uint8_t *)a.out + bytes) return (int)hipErrorInvalidValue;
    if (a.lower != nullptr && (a.out != a.fb || a.lower != a.fbclean)) return (int)hipErrorInvalidValue;
    a.total = layer_block_bytes(q.width, q.height, q.stride, q.format);
    if (a.image && a.image < (const uint8_t *)a.out + bytes && (const uint8_t *)a.out < a.image + a.total) return (int)hipErrorInvalidValue;
    // the rectangle clipped to the frame, in 64 bits: x + width may pass 2^31
    const int64_t cx0 = std::max<int64_t>(0, q.x), cx1 = std::min<int64_t>(W, (int64_t)q.x + q.width);
    const int64_t cr0 = std::max<int64_t>(0, q.y), cr1 = std::min<int64_t>(H, (int64_t)q.y + q.height);
    const bool miss = cx0 >= cx1 || cr0 >= cr1;
    a.cx0 = miss ? 0 : (int32_t)cx0, a.cx1 = miss ? 0 : (int32_t)cx1, a.cr0 = miss ? 0 : (int32_t)cr0, a.cr1 = miss ? 0 : (int32_t)cr1;
    if (miss) a.rule.x = a.rule.y = 0;  // (never looked at; keeps the kernel's 32-bit differences small)
    if (a.out == a.fb) {
        // in place: the tiles the rectangle touches (tile rows count from the bottom)
        if (miss || q.opacity == 0u) return 0;
        a.gx0 = (uint32_t)cx0 / TILE_W, a.gnx = (uint32_t)(cx1 - 1) / TILE_W - a.gx0 + 1u;
        a.gy0 = (H - (uint32_t)cr1) / TILE_H, a.gny = (H - 1u - (uint32_t)cr0) / TILE_H - a.gy0 + 1u;
    } else {
        a.gx0 = a.gy0 = 0u, a.gnx = a.frame.ntx, a.gny = a.frame.nty;
    }
    // whole words: every unit of four pixels is three aligned words of either buffer, its depths one 16-byte piece
    const bool words = W % 4u == 0u && ((uintptr_t)a.fb | (uintptr_t)a.out) % 4u == 0u && (where_flags == 0u || (uintptr_t)a.z % 16u == 0u);
    const bool where = where_flags != 0u;
#define LAYER_LAUNCH(FORMAT_)                                        \
    {                                                                \
        if (words) launch_layer_form<true, FORMAT_>(a, where, st);   \
        else launch_layer_form<false, FORMAT_>(a, where, st);        \
    }
    if (from_scene) LAYER_LAUNCH(LAYER_FROM_SCENE)
    else if (q.format == LAYER_RGBA8) LAYER_LAUNCH((int)LAYER_RGBA8)
    else LAYER_LAUNCH((int)LAYER_RGB8)
#undef LAYER_LAUNCH
    TR_LAUNCH_CHECK();
    return 0;
}

int launch_projector(const ProjectorArgs &a, hipStream_t st)
{
    const uint32_t W = a.frame.width, H = a.frame.height, n_tiles = a.frame.ntx * a.frame.nty;
    if (n_tiles == 0) return 0;
    const ProjectorRule &q = a.rule;
    if (!a.fb || !a.out || !a.z || !a.zclean || !a.image) return (int)hipErrorInvalidValue;
    // the whole frame's tile grid (both flag sets and z are indexed by it), the rule's limits
    if (a.frame.ty_base != 0 || a.frame.band_y0 != 0 || a.frame.band_y1 != (int32_t)H) return (int)hipErrorInvalidValue;
    if (a.frame.ntx != (W + TILE_W - 1) / TILE_W || a.frame.nty != (H + TILE_H - 1) / TILE_H) return (int)hipErrorInvalidValue;
    if (q.pw < 1u || q.pw > PROJECTOR_MAX_SIDE || q.ph < 1u || q.ph > PROJECTOR_MAX_SIDE || (q.bpp != 3u && q.bpp != 4u) || q.stride < q.pw * q.bpp ||
        q.mode >= LAYER_MODES || q.opacity > 256u || (q.flags & ~(PROJECTOR_OCCLUDE | PROJECTOR_SOFT)) != 0u || q.flags == PROJECTOR_SOFT)
        return (int)hipErrorInvalidValue;
    // the occluder: its depth and its flags over its own tile grid
    if ((q.flags & PROJECTOR_OCCLUDE) && (!a.occ_z || !a.occ_zclean || a.occ_ntx != (q.pw + TILE_W - 1) / TILE_W)) return (int)hipErrorInvalidValue;
    // `out` is the frame itself or apart from it; a flag is lowered in place only; the image is apart from both
    const size_t bytes = (size_t)W * H * 3u;
    if (a.out != a.fb && (const uint8_t *)a.out < a.fb + bytes && a.fb < (const uint8_t *)a.out + bytes) return (int)hipErrorInvalidValue;
    if (a.lower != nullptr && (a.out != a.fb || a.lower != a.fbclean)) return (int)hipErrorInvalidValue;
    if (a.image < (const uint8_t *)a.out + bytes && (const uint8_t *)a.out < a.image + projector_image_bytes(q)) return (int)hipErrorInvalidValue;
    // whole words: every unit of four pixels is three aligned words of either buffer, its depths one 16-byte piece
    const bool words = W % 4u == 0u && ((uintptr_t)a.fb | (uintptr_t)a.out) % 4u == 0u && (uintptr_t)a.z % 16u == 0u;
    if (words)
        hipLaunchKernelGGL((k_projector<true>), dim3(n_tiles), dim3(PROJECTOR_THREADS), 0, st, a);
    else
        hipLaunchKernelGGL((k_projector<false>), dim3(n_tiles), dim3(PROJECTOR_THREADS), 0, st, a);
    TR_LAUNCH_CHECK();
    return 0;
}

int launch_relight(const RelightArgs &a, hipStream_t st)
{
    const uint32_t W = a.frame.width, H = a.frame.height, n_tiles = a.frame.ntx * a.frame.nty;
    if (n_tiles == 0) return 0;
    const RelightRule &q = a.rule;
    if (!a.fb || !a.out || !a.z || !a.zclean) return (int)hipErrorInvalidValue;
    // the whole frame's tile grid (both flag sets and z are indexed by it), the rule's limits
    if (a.frame.ty_base != 0 || a.frame.band_y0 != 0 || a.frame.band_y1 != (int32_t)H) return (int)hipErrorInvalidValue;
    if (a.frame.ntx != (W + TILE_W - 1) / TILE_W || a.frame.nty != (H + TILE_H - 1) / TILE_H) return (int)hipErrorInvalidValue;
    if (q.mode >= LAYER_MODES || q.opacity > 256u || (q.flags & ~(RELIGHT_ALBEDO | RELIGHT_SHOW_NORMALS)) != 0u || q.n_lights > RELIGHT_MAX_LIGHTS)
        return (int)hipErrorInvalidValue;
    for (uint32_t l = 0; l < q.n_lights; l++)
        if (q.lights[l].kind > RELIGHT_SPOT || q.lights[l].shininess_log2 > RELIGHT_MAX_SHININESS_LOG2) return (int)hipErrorInvalidValue;
    // `out` is the frame itself or apart from it; a flag is lowered in place only
    const size_t bytes = (size_t)W * H * 3u;
    if (a.out != a.fb && (const uint8_t *)a.out < a.fb + bytes && a.fb < (const uint8_t *)a.out + bytes) return (int)hipErrorInvalidValue;
    if (a.lower != nullptr && (a.out != a.fb || a.lower != a.fbclean)) return (int)hipErrorInvalidValue;
    // whole words: every unit of four pixels is three aligned words of either buffer, its depths one 16-byte piece
    const bool wide = W % 4u == 0u && ((uintptr_t)a.fb | (uintptr_t)a.out) % 4u == 0u && (uintptr_t)a.z % 16u == 0u;
    if (wide)
        hipLaunchKernelGGL((k_relight<true>), dim3(n_tiles), dim3(RELIGHT_THREADS), 0, st, a);
    else
        hipLaunchKernelGGL((k_relight<false>), dim3(n_tiles), dim3(RELIGHT_THREADS), 0, st, a);
    TR_LAUNCH_CHECK();
    return 0;
}

int launch_lines(const LinesArgs &a_in, uint32_t n_listed, hipStream_t st)
{
    LinesArgs a = a_in;
    const uint32_t W = a.frame.width, H = a.frame.height, n_tiles = a.frame.ntx * a.frame.nty;
    if (n_tiles == 0) return 0;
    if (!a.fb || !a.out || !a.lines || !a.offsets || !a.entries || !a.tiles || n_listed > n_tiles) return (int)hipErrorInvalidValue;
    // the whole frame's tile grid (the flags and the lists are indexed by it), the rule's limits
    if (a.frame.ty_base != 0 || a.frame.band_y0 != 0 || a.frame.band_y1 != (int32_t)H) return (int)hipErrorInvalidValue;
    if (a.frame.ntx != (W + TILE_W - 1) / TILE_W || a.frame.nty != (H + TILE_H - 1) / TILE_H) return (int)hipErrorInvalidValue;
    const LinesRule &q = a.rule;
    if (q.width < 1u || q.width > LINES_MAX_WIDTH || q.opacity > 256u || (q.flags & ~(LINES_DEPTH_TEST | LINES_PAINTER)) != 0u) return (int)hipErrorInvalidValue;
    const bool test = (q.flags & LINES_DEPTH_TEST) != 0u;
    if (test && (!a.z || !a.zclean)) return (int)hipErrorInvalidValue;
    // `out` is the frame itself or apart from it; a flag is lowered in place only
    const size_t bytes = (size_t)W * H * 3u;
    if (a.out != a.fb && (const uint8_t *)a.out < a.fb + bytes && a.fb < (const uint8_t *)a.out + bytes) return (int)hipErrorInvalidValue;
    if (a.lower != nullptr && (a.out != a.fb || a.lower != a.fbclean)) return (int)hipErrorInvalidValue;
    uint32_t grid = n_tiles;
    if (a.out == a.fb) {
        // in place: the non-empty tiles, one workgroup each
        if (n_listed == 0u || q.opacity == 0u) return 0;
        grid = n_listed;
    } else {
        a.tiles = nullptr;  // (workgroup t takes tile t: the tiles without a list are copied)
    }
    // whole words: every unit of four pixels is three aligned words of either buffer
    const bool words = W % 4u == 0u && ((uintptr_t)a.fb | (uintptr_t)a.out) % 4u == 0u;
    if (words && test) hipLaunchKernelGGL((k_lines<true, true>), dim3(grid), dim3(LINES_THREADS), 0, st, a);
    else if (words) hipLaunchKernelGGL((k_lines<true, false>), dim3(grid), dim3(LINES_THREADS), 0, st, a);
    else if (test) hipLaunchKernelGGL((k_lines<false, true>), dim3(grid), dim3(LINES_THREADS), 0, st, a);
    else hipLaunchKernelGGL((k_lines<false, false>), dim3(grid), dim3(LINES_THREADS), 0, st, a);
    TR_LAUNCH_CHECK();
    return 0;
}

int launch_outline(const OutlineArgs &a, hipStream_t st)
{
    const uint32_t n_tiles = a.frame.ntx * a.frame.nty;
    if (n_tiles == 0) return 0;
    if (!a.z || !a.zclean || !a.fb || !a.fbclean || !a.out) return (int)hipErrorInvalidValue;
    // the whole frame's tile grid (a band's halo would lie on another rank), seeds inside the staged halo
    if (a.frame.ty_base != 0 || a.frame.band_y0 != 0 || a.frame.band_y1 != (int32_t)a.frame.height) return (int)hipErrorInvalidValue;
    if (a.rule.radius > (uint32_t)OUTLINE_MAX_RADIUS || a.rule.opacity > 256u || (a.rule.flags & ~(OUTLINE_CREASES | OUTLINE_ONLY)) != 0u)
        return (int)hipErrorInvalidValue;
    // `out` is the frame itself or apart from it
    const size_t bytes = (size_t)a.frame.width * a.frame.height * 3u;
    if (a.out != a.fb && (const uint8_t *)a.out < a.fb + bytes && a.fb < (const uint8_t *)a.out + bytes) return (int)hipErrorInvalidValue;
    // the wide path: z in aligned 16-byte pieces, every unit of four pixels three aligned words of either buffer
    const bool wide = a.frame.width % 4u == 0u && (uintptr_t)a.z % 16u == 0u && ((uintptr_t)a.fb | (uintptr_t)a.out) % 4u == 0u;
    if (wide)
        hipLaunchKernelGGL((k_outline<true>), dim3(n_tiles), dim3(OUTLINE_THREADS), 0, st, a);
    else
        hipLaunchKernelGGL((k_outline<false>), dim3(n_tiles), dim3(OUTLINE_THREADS), 0, st, a);
    TR_LAUNCH_CHECK();
    return 0;
}

int launch_aa(const AaArgs &a, hipStream_t st)
{
    const uint32_t n_tiles = a.frame.ntx * a.frame.nty;
    if (n_tiles == 0) return 0;
    if (!a.fb || !a.out) return (int)hipErrorInvalidValue;
    // the whole frame's tile grid (a band's halo would lie on another rank), the search inside the staged halo
    if (a.frame.ty_base != 0 || a.frame.band_y0 != 0 || a.frame.band_y1 != (int32_t)a.frame.height) return (int)hipErrorInvalidValue;
    if (a.frame.ntx != (a.frame.width + TILE_W - 1) / TILE_W || a.frame.nty != (a.frame.height + TILE_H - 1) / TILE_H) return (int)hipErrorInvalidValue;
    if (a.rule.search < 1u || a.rule.search > (uint32_t)AA_MAX_SEARCH || a.rule.contrast_min > 255u || a.rule.contrast_rel > 256u ||
        a.rule.subpixel > 256u || (a.rule.flags & ~AA_SHOW_BLEND) != 0u)
        return (int)hipErrorInvalidValue;
    // `out` is apart from the frame
    const size_t bytes = (size_t)a.frame.width * a.frame.height * 3u;
    if ((const uint8_t *)a.out < a.fb + bytes && a.fb < (const uint8_t *)a.out + bytes) return (int)hipErrorInvalidValue;
    // the wide path: every unit of four pixels three aligned words of either buffer
    const bool wide = a.frame.width % 4u == 0u && ((uintptr_t)a.fb | (uintptr_t)a.out) % 4u == 0u;
    if (wide)
        hipLaunchKernelGGL((k_aa<true>), dim3(n_tiles), dim3(AA_THREADS), 0, st, a);
    else
        hipLaunchKernelGGL((k_aa<false>), dim3(n_tiles), dim3(AA_THREADS), 0, st, a);
    TR_LAUNCH_CHECK();
    return 0;
}

template <int I>
static void launch_resize_shape(const ResizeArgs &a, bool wide, hipStream_t st)
{
    constexpr ResizeShape S = kResizeShapes[I];
    const dim3 grid((a.out_w + S.w - 1) / S.w, (a.out_h + S.h - 1) / S.h);
    if (wide)
        hipLaunchKernelGGL((k_resize<S.w, S.h, S.rows, true>), grid, dim3(RESIZE_THREADS), 0, st, a);
    else
        hipLaunchKernelGGL((k_resize<S.w, S.h, S.rows, false>), grid, dim3(RESIZE_THREADS), 0, st, a);
}

int launch_resize(const ResizeArgs &a, hipStream_t st)
{
    if (!a.fb || !a.out || !a.x.fc || !a.x.w || !a.y.fc || !a.y.w) return (int)hipErrorInvalidValue;
    // the whole frame's tile grid (the flags are indexed by it), the rule's limits, a shape the tables fit
    if (a.frame.ty_base != 0 || a.frame.band_y0 != 0 || a.frame.band_y1 != (int32_t)a.frame.height) return (int)hipErrorInvalidValue;
    if (a.frame.ntx != (a.frame.width + TILE_W - 1) / TILE_W || a.frame.nty != (a.frame.height + TILE_H - 1) / TILE_H) return (int)hipErrorInvalidValue;
    if (!resize_side_ok(a.frame.width, a.out_w) || !resize_side_ok(a.frame.height, a.out_h)) return (int)hipErrorInvalidValue;
    if (a.shape < 0 || a.shape >= RESIZE_SHAPES || a.y_span > (uint32_t)kResizeShapes[a.shape].rows) return (int)hipErrorInvalidValue;
    if (a.x_span > (uint32_t)(RESIZE_FLAGS_W - 1) * TILE_W + 1u || (uintptr_t)a.x.w % 16u != 0u) return (int)hipErrorInvalidValue;
    // `out` is apart from the frame
    const size_t bytes = (size_t)a.frame.width * a.frame.height * 3u, out_bytes = (size_t)a.out_w * a.out_h * 3u;
    if ((const uint8_t *)a.out < a.fb + bytes && a.fb < (const uint8_t *)a.out + out_bytes) return (int)hipErrorInvalidValue;
    // the wide path: every unit of four output pixels three aligned words
    const bool wide = a.out_w % 4u == 0u && (uintptr_t)a.out % 4u == 0u;
    if (a.shape == 0) launch_resize_shape<0>(a, wide, st);
    else if (a.shape == 1) launch_resize_shape<1>(a, wide, st);
    else launch_resize_shape<2>(a, wide, st);
    TR_LAUNCH_CHECK();
    return 0;
}

template <uint32_t LAYOUT>
static void launch_yuv_layout(const YuvArgs &a, int n, hipStream_t st)
{
    const dim3 grid((a.width + YUV_BW - 1) / YUV_BW, (a.height + YUV_BH - 1) / YUV_BH);
    if (n == 8) hipLaunchKernelGGL((k_yuv<8, LAYOUT>), grid, dim3(128), 0, st, a);
    else if (n == 4) hipLaunchKernelGGL((k_yuv<4, LAYOUT>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_yuv<2, LAYOUT>), grid, dim3(256), 0, st, a);
}

int launch_yuv(const YuvArgs &a, hipStream_t st)
{
    if (!a.src || !a.out) return (int)hipErrorInvalidValue;
    if (a.width < 1u || a.width > YUV_MAX_SIDE || a.height < 1u || a.height > YUV_MAX_SIDE || !yuv_layout_ok(a.rule.layout)) return (int)hipErrorInvalidValue;
    // flags are indexed by the whole image's tile grid
    if (a.clean && a.ntx != (a.width + TILE_W - 1) / TILE_W) return (int)hipErrorInvalidValue;
    // `out` is apart from the source
    const size_t bytes = (size_t)a.width * a.height * 3u, out_bytes = yuv_bytes(a.width, a.height, a.rule.layout);
    if ((const uint8_t *)a.out < a.src + bytes && a.src < (const uint8_t *)a.out + out_bytes) return (int)hipErrorInvalidValue;
    // the unit: 8 or 4 columns where every load and store of that form is aligned, else 2 columns by bytes
    const uintptr_t both = (uintptr_t)a.src | (uintptr_t)a.out;
    const int n = a.width % 8u == 0u && both % 8u == 0u ? 8 : a.width % 4u == 0u && both % 4u == 0u ? 4 : 2;
    if (a.rule.layout == YUV_I420) launch_yuv_layout<YUV_I420>(a, n, st);
    else if (a.rule.layout == YUV_NV12) launch_yuv_layout<YUV_NV12>(a, n, st);
    else launch_yuv_layout<YUV_I444>(a, n, st);
    TR_LAUNCH_CHECK();
    return 0;
}

int launch_warp(const WarpArgs &a, hipStream_t st)
{
    if (!a.fb || !a.out || !a.grid || (uintptr_t)a.grid % 8u != 0u) return (int)hipErrorInvalidValue;
    // the whole frame's tile grid (the flags are indexed by it), the rule's limits
    if (a.frame.ty_base != 0 || a.frame.band_y0 != 0 || a.frame.band_y1 != (int32_t)a.frame.height) return (int)hipErrorInvalidValue;
    if (a.frame.ntx != (a.frame.width + TILE_W - 1) / TILE_W || a.frame.nty != (a.frame.height + TILE_H - 1) / TILE_H) return (int)hipErrorInvalidValue;
    if (a.frame.width < 1u || a.frame.height < 1u) return (int)hipErrorInvalidValue;
    if (a.out_w < 1u || a.out_w > WARP_MAX_SIDE || a.out_h < 1u || a.out_h > WARP_MAX_SIDE) return (int)hipErrorInvalidValue;
    if (a.rule.edge > WARP_CLAMP || a.rule.border[0] > 255u || a.rule.border[1] > 255u || a.rule.border[2] > 255u) return (int)hipErrorInvalidValue;
    // `out` is apart from the frame; flags of `out` only where its tiles are the frame's
    const size_t bytes = (size_t)a.frame.width * a.frame.height * 3u, out_bytes = (size_t)a.out_w * a.out_h * 3u;
    if ((const uint8_t *)a.out < a.fb + bytes && a.fb < (const uint8_t *)a.out + out_bytes) return (int)hipErrorInvalidValue;
    if (a.out_clean && (a.out_w != a.frame.width || a.out_h != a.frame.height || a.frame.height % TILE_H != 0u)) return (int)hipErrorInvalidValue;
    // the wide path: every unit of four output pixels three aligned words
    const bool wide = a.out_w % 4u == 0u && (uintptr_t)a.out % 4u == 0u;
    const dim3 grid((a.out_w + WARP_TW - 1) / WARP_TW, (a.out_h + WARP_TH - 1) / WARP_TH);
    if (a.rule.per_channel) {
        if (wide) hipLaunchKernelGGL((k_warp<true, true>), grid, dim3(WARP_THREADS), 0, st, a);
        else hipLaunchKernelGGL((k_warp<true, false>), grid, dim3(WARP_THREADS), 0, st, a);
    } else {
        if (wide) hipLaunchKernelGGL((k_warp<false, true>), grid, dim3(WARP_THREADS), 0, st, a);
        else hipLaunchKernelGGL((k_warp<false, false>), grid, dim3(WARP_THREADS), 0, st, a);
    }
    TR_LAUNCH_CHECK();
    return 0;
}

uint32_t stats_max_grid(const DevFrame &frame)
{
    const uint32_t n_tiles = frame.ntx * frame.nty;
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
        return 0u;
    // one workgroup of 1024 lanes a CU, and no more workgroups than tiles
    return std::max<uint32_t>(1u, std::min<uint32_t>((uint32_t)cus, n_tiles));
}

int launch_stats(const StatsArgs &a, uint32_t *out, hipStream_t st, uint32_t cap, uint32_t *grid_out)
{
    *grid_out = 0u;
    if (!a.fb || !a.partials || !out || (uintptr_t)a.partials % 16u != 0u || (uintptr_t)out % 4u != 0u) return (int)hipErrorInvalidValue;
    const bool depth = a.rule.depth != 0u;
    if (depth && a.cleared == 0u && (!a.z || !a.zclean)) return (int)hipErrorInvalidValue;
    // the window lies inside the frame and the band (an empty one is served: every workgroup stores zeros)
    const StatsWindow &w = a.rule.win;
    if (w.x0 < 0 || w.x1 > (int32_t)a.frame.width || w.y0 < a.frame.band_y0 || w.y1 > a.frame.band_y1) return (int)hipErrorInvalidValue;
    if (a.frame.band_y0 < 0 || a.frame.band_y1 > (int32_t)a.frame.height) return (int)hipErrorInvalidValue;
    uint32_t grid = stats_max_grid(a.frame);
    if (grid == 0u) return (int)hipErrorInvalidDevice;
    if (cap != 0u) grid = std::min<uint32_t>(grid, cap);  // (the diagnostic: fewer workgroups, more rounds each)
    *grid_out = grid;
    // whole words: every unit of four pixels is three aligned words of colour and one aligned 16-byte piece of depth
    const bool words = a.frame.width % 4u == 0u && (uintptr_t)a.fb % 4u == 0u && (!depth || a.cleared != 0u || (uintptr_t)a.z % 16u == 0u);
    if (depth && words)
        hipLaunchKernelGGL((k_stats<true, true>), dim3(grid), dim3(STATS_THREADS), 0, st, a);
    else if (depth)
        hipLaunchKernelGGL((k_stats<true, false>), dim3(grid), dim3(STATS_THREADS), 0, st, a);
    else if (words)
        hipLaunchKernelGGL((k_stats<false, true>), dim3(grid), dim3(STATS_THREADS), 0, st, a);
    else
        hipLaunchKernelGGL((k_stats<false, false>), dim3(grid), dim3(STATS_THREADS), 0, st, a);
    TR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_stats_finish, dim3(STATS_FINISH_BLOCKS), dim3(STATS_FINISH_THREADS), 0, st, (const uint32_t *)a.partials, grid, a.rule.depth, out);
    TR_LAUNCH_CHECK();
    return 0;
}

int launch_accumulate(const AccumulateArgs &a, hipStream_t st)
{
    const uint32_t n_tiles = a.frame.ntx * a.frame.nty;
    if (n_tiles == 0) return 0;
    if (!a.out || a.n == 0u || a.n > ACC_MAX_FRAMES || a.div.mul == 0u) return (int)hipErrorInvalidValue;
    // the wide path: every share is whole 16-byte pieces of every buffer
    uintptr_t low_bits = (uintptr_t)a.out;
    for (uint32_t k = 0; k < a.n; k++) {
        if (!a.fb[k] || a.w[k] > ACC_MAX_WEIGHT) return (int)hipErrorInvalidValue;
        low_bits |= (uintptr_t)a.fb[k];
    }
    const bool wide = a.frame.width % 16u == 0u && low_bits % 16u == 0u;
    if (wide)
        hipLaunchKernelGGL((k_accumulate<true>), dim3(n_tiles), dim3(8 * TILE_H), 0, st, a);
    else
        hipLaunchKernelGGL((k_accumulate<false>), dim3(n_tiles), dim3(8 * TILE_H), 0, st, a);
    TR_LAUNCH_CHECK();
    return 0;
}

int launch_pack_texels(const PackArgs &a, int words, hipStream_t st)
{
    if (a.w == 0u || a.h == 0u) return 0;
    if (!a.texel || (!a.src && !a.src_all_clean) || (a.set && words != 1 && words != 4)) return (int)hipErrorInvalidValue;
    if (a.set && ((a.mode == PACK_SPEC && !a.other) || (a.mode != 0u && a.mode != PACK_COLOUR && words != 4))) return (int)hipErrorInvalidValue;
    const uint32_t ntx = (a.w + (uint32_t)TILE_W - 1u) / (uint32_t)TILE_W, nty = (a.h + (uint32_t)TILE_H - 1u) / (uint32_t)TILE_H;
    const dim3 grid(ntx * nty * ((uint32_t)TILE_H / PACK_ROWS)), block(256);
    // the wide path: a quad is three aligned dwords of the source and one aligned 16-byte word of each plain array
    const bool wide = a.w % PACK_QUAD == 0u && (uintptr_t)a.src % 4u == 0u && ((uintptr_t)a.texel | (uintptr_t)a.other) % 16u == 0u;
    if ((uintptr_t)a.set % 16u) return (int)hipErrorInvalidValue;
    if (a.set && words == 4) {
        if (wide) hipLaunchKernelGGL((k_pack_texels<4, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_pack_texels<4, false>), grid, block, 0, st, a);
    } else {
        if (wide) hipLaunchKernelGGL((k_pack_texels<1, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_pack_texels<1, false>), grid, block, 0, st, a);
    }
    TR_LAUNCH_CHECK();
    return 0;
}

int launch_morph(const float *base, const float *delta, uint32_t n_rows, uint32_t n_targets, const MorphTable &tab, uint32_t n_frames,
                 hipStream_t st, hipEvent_t start, hipEvent_t done)
{
    if (n_rows == 0 || n_frames == 0) return 0;
    if (n_frames > (uint32_t)MORPH_MAX_FRAMES || n_rows > 0xFFFFFFFFu / 6u) return (int)hipErrorInvalidValue;
    const uint32_t n_pieces = n_rows * 6u;  // 16-byte pieces of the rows
    const dim3 grid((n_pieces + 255u) / 256u, n_frames);
    hipExtLaunchKernelGGL(k_morph, grid, dim3(256), 0, st, start, done, 0, reinterpret_cast<const float4 *>(base),
                          reinterpret_cast<const float4 *>(delta), n_pieces, n_targets, tab);
    TR_LAUNCH_CHECK();
    return 0;
}

int launch_skin(const uint32_t *infl, uint32_t n_rows, uint32_t n_bones, const SkinTable &tab, uint32_t n_frames, hipStream_t st,
                hipEvent_t start, hipEvent_t done)
{
    if (n_rows == 0 || n_frames == 0) return 0;
    if (n_frames > (uint32_t)SKIN_MAX_FRAMES || n_bones == 0 || n_bones > (uint32_t)SKIN_MAX_BONES) return (int)hipErrorInvalidValue;
    const dim3 grid((n_rows + 255u) / 256u, n_frames);
    hipExtLaunchKernelGGL(k_skin, grid, dim3(256), 0, st, start, done, 0, reinterpret_cast<const uint4 *>(infl), n_rows, n_bones, tab);
    TR_LAUNCH_CHECK();
    return 0;
}

int launch_selftest_shadow(const float *plain, const float *stale, const uint32_t *sclean, uint32_t W, uint32_t H,
                           const float *x, const float *y, uint32_t n, uint32_t *out_plain, uint32_t *out_flagged,
                           uint32_t *err_plain, uint32_t *err_flagged, hipStream_t st)
{
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_selftest_shadow, dim3((n + 255u) / 256u), dim3(256), 0, st, plain, stale, sclean, W, H, x, y, n,
                       out_plain, out_flagged, err_plain, err_flagged);
    TR_LAUNCH_CHECK();
    return 0;
}

int specular_is_exact() { return TR_POWF_EXACT; }

int launch_depth_view(const float *src, uint8_t *dst, uint32_t W, uint32_t H, hipStream_t st)
{
    const size_t n = (size_t)W * H;
    if (n == 0) return 0;
    size_t blocks = (n + 255u) / 256u;
    if (blocks > 8192u) blocks = 8192u;
    hipLaunchKernelGGL(k_depth_view, dim3((uint32_t)blocks), dim3(256), 0, st, src, dst, W, H);
    TR_LAUNCH_CHECK();
    return 0;
}

}  // namespace tr
