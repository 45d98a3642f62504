// tr_scene.cpp -- host side of the C ABI: scene state, pass sequencing, buffer ownership.
//
// Mirrors the role of the reference's `Scene` (src/scene.rs:25-269) and `ShaderPipeline`
// registry (src/scene/shader.rs:97-112) for a device-resident frame: the model, textures,
// z / shadow / frame buffers live in HBM for the life of the scene; a frame is a handful of
// kernel launches on one HIP stream and nothing is copied unless a getter is called.
//
// There is no CPU rendering path in this library.  If HIP or a gfx950 device is not usable,
// tr_scene_create fails with TR_E_HIP.
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "tiny_renderer.h"
#include "tr_error.h"
#include "tr_kernels.h"
#include "tr_math.h"
#include "tr_pack.h"
#include "tr_plan.h"
#include "tr_powf.h"
#include "tr_prepare.h"
#include "tr_shaders.h"
#include "tr_texels.h"
#include "tr_types.h"

namespace tr {

namespace {
thread_local std::string g_last_error;
}

int fail(int code, const std::string &msg)
{
    g_last_error = msg;
    return code;
}

}  // namespace tr

using namespace tr;

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return tr::fail(TR_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));      \
    } while (0)

namespace {

// Page-locked host buffers handed out by tr_host_alloc: host address -> {bytes, device address of the mapping}
struct HostAlloc {
    size_t bytes;
    void *device;
    uint64_t serial;  // (an address can come back from a later allocation: what a scene remembers is about THIS one)
    // Who wrote the buffer last, and how often anybody has: a scene's record of the buffer's zero tiles (HostFlags)
    // holds only while that scene was the last writer and nobody has written since -- another scene reading back
    // into the same buffer, or tr_scene_host_buffer_written, moves `gen` on and every record of the buffer lapses
    uint64_t writer;
    uint64_t gen;
};
std::mutex g_host_mutex;
uint64_t g_host_serial = 0;
uint64_t g_scene_serial = 0;  // tr_scene::id
std::map<void *, HostAlloc> g_host_allocs;

struct PassDesc {
    int prepare_kind;  // 0 default_prepare, 1 shadow_pass_prepare_1, 2 shadow_pass_prepare_2
    int vs, fs;
};

struct PipelineDesc {
    const char *name;
    int n_passes;
    PassDesc pass[2];
};

// shader.rs:100-109 and the pass lists of shader.rs:282-963
const PipelineDesc kPipelines[P_COUNT] = {
    { "default", 1, { { 0, VS_DEFAULT, FS_DEFAULT }, {} } },
    { "phong", 1, { { 0, VS_PHONG, FS_PHONG }, {} } },
    { "normal_map", 1, { { 0, VS_PLAIN, FS_NORMAL_MAP }, {} } },
    { "specular", 1, { { 0, VS_PLAIN, FS_SPECULAR }, {} } },
    { "darboux", 1, { { 0, VS_DARBOUX, FS_DARBOUX }, {} } },
    { "shadow", 2, { { 1, VS_DEPTH, FS_DEPTH }, { 2, VS_PHONG, FS_SHADOW2 } } },
    { "occlusion", 2, { { 1, VS_DEPTH, FS_DEPTH }, { 2, VS_PLAIN, FS_OCCLUSION2 } } },
};

const char *kKernelNames[] = { "k_setup", "k_tile", "k_tile_depth", "k_clear", "k_order", "k_bin", "k_lit", "k_resolve", "k_morph", "k_skin", "k_composite", "k_ao", "k_accumulate", "k_dof", "k_shadow_merge", "k_pack_texels", "k_bloom", "k_grade", "k_stats", "k_outline", "k_aa", "k_resize", "k_warp", "k_convolve", "k_yuv", "k_layer", "k_rank", "k_ramp", "k_bilateral", "k_dist", "k_dist_apply", "k_lines" };
enum KernelId { K_SETUP = 0, K_TILE, K_TILE_DEPTH, K_CLEAR, K_ORDER, K_BIN, K_LIT, K_RESOLVE, K_MORPH, K_SKIN, K_COMPOSITE, K_AO, K_ACCUMULATE, K_DOF, K_SHADOW_MERGE, K_PACK_TEXELS, K_BLOOM, K_GRADE, K_STATS, K_OUTLINE, K_AA, K_RESIZE, K_WARP, K_CONVOLVE, K_YUV, K_LAYER, K_RANK, K_RAMP, K_BILATERAL, K_DIST, K_DIST_APPLY, K_LINES, K_COUNT };

struct EventPair {
    hipEvent_t a, b;
    int kernel;
    uint32_t frames;  // frames the launch covered (fused launches of tr_scene_render_frames: more than one)
};

}  // namespace

// How many passes the setup stream may run ahead of the tile kernels: setup of pass p waits for the
// tile kernel of pass p - LOOKAHEAD only.  With 2 the setup chain (k_setup, k_order_count,
// k_order_place: ~35 us beside a busy machine) had to fit inside one tile kernel (~34 us) and was
// the critical path of the frame loop; 3 gave it two (44.1 -> 42.4 us per frame); 5 lets four passes
// wait on the host for their setups to finish, so that their tile kernels need no wait packet (below).
// Costs LOOKAHEAD sets of bins (0.2 GB each at 4096^2) -- cheap next to 288 GB.
using tr::plan::LOOKAHEAD;   // (tr_plan.h: the decisions of this file live there, testable without a GPU)
constexpr uint64_t LIT_PIXELS_PER_TEXEL = 16;  // frame pixels per image texel from which the lit path (k_lit) is taken
constexpr int SETS = LOOKAHEAD + 1;
// Handing tile kernels to the main stream.  The tile kernel of pass p must run after that pass's setup
// (other stream).  A cross-stream wait packet sitting between two tile kernels in the main stream's
// queue costs 5.5 us (two back-to-back tile kernels are 3.8 us apart, 9.3 with the wait in between), and
// none is needed if the setup has ALREADY completed when the tile kernel is enqueued.  So a pass whose
// setup is queued stays "pending" on the host until one of these:
//   * more than BATCH passes are pending (the steady state of a running loop): the host waits for the
//     oldest one's setup event itself -- it has completed or is about to, the setup stream runs ahead --
//     and enqueues its tile kernel with no wait packet at all.  That host-side wait is also the
//     frames-in-flight limit: render() cannot run more than BATCH + LOOKAHEAD passes ahead of the GPU;
//   * its setup event reads complete at a later render(): out it goes, no wait (start-up);
//   * the main stream has run dry (its newest tile kernel has completed): the oldest pending pass goes
//     out behind a wait packet on ITS setup event -- the first frame after a sync;
//   * anything needs the main stream or waits for the scene -- a getter, a sync, a clear that must be
//     materialised, a read-back, destruction: everything pending goes out behind ONE wait for the newest
//     setup (the setup stream is in order).
// BATCH <= LOOKAHEAD - 1: the setup of pass p waits for the tile kernel of pass p - LOOKAHEAD, which must
// have been submitted by then.  Nothing observable changes (submit_pending runs before every use of the
// stream).  Round 1 handed over in fixed batches of four behind one wait packet: 35.2 us/frame where this
// gives 34.2 (same box), and at small frames 25 -> 20.5 us (800^2), 24.8 -> 22.4 (2048^2).
using tr::plan::BATCH;  // passes that may be pending (setup queued, tile kernel not yet)
constexpr int RING = 16;  // events: pass p's are waited for until pass p + LOOKAHEAD is set up
constexpr size_t ORDER_LISTS = 8;  // k_order's work lists per pass, n_tiles entries each (tr_kernels.hip)

// Frame groups (tr_scene_render_frames).  A lone frame cannot keep the GPU full: at 4096^2 a third of the tile
// kernel runs on a machine that is draining (2 168 busy tiles on 1 536 workgroup slots), and smaller frames never
// fill it at all; kernels of different launches do not overlap on this stack (profiles/r02_notes.md).  So the
// frames of a group are rendered by ONE launch per kernel -- vertex stage + binning, work lists, tiles -- each
// frame into a frame slot of its own (z, colour, fast-clear flags, shadow buffer).  Same replicated frame,
// k_tile per frame (us, group of 1 / 2 / 4 / 8): 4096^2 phong 33.9 / 29.0 / 27.0 / 27.0, darboux 65.9 / 59.5 /
// 58.9 / 56.3, 2048^2 phong 21.3 / 14.2 / 12.6 / 12.0, 800^2 26.3 / 12.8 / 7.4 / 4.5, 512^2 22.5 / 12.2 / 6.6 / 3.6.
using tr::plan::GROUP_MAX;   // frames per fused launch, at most
using tr::plan::GROUP_SETS;  // groups in flight: group g's setup reuses the bins of group g - GROUP_SETS
constexpr size_t LEN_WORDS = 8;  // a pass's words in GroupSet::h_lens: its eight list lengths

struct tr_scene {
    uint64_t id = 0;  // unique per scene of the process (who wrote a tr_host_alloc buffer last)
    uint32_t width = 0, height = 0;
    int pipeline = 0;
    int device = 0;
    uint32_t flags = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;

    // The view the next render draws under: light direction and camera (Scene::new defaults, scene.rs:66-69)
    tr_frame_params view = { { 0.0f, 0.0f, -1.0f }, { 0.0f, 0.0f, 1.0f }, { 0.0f, 0.0f, 0.0f }, { 0.0f, 1.0f, 0.0f } };

    DevMesh mesh = {};         // what a pass rendered now draws: the mesh under the current instance table
    DevTextures tex = {};
    // Instance tables (tr_scene_set_instances).  A table is copied to the device once, into a block that is never
    // written again while anybody may render with it: the scene's current table, frames held back, the frames a
    // replay or a depth-only repeat may render again (InstRef), and work already queued -- each block has one event
    // per stream that the chains reading it run on, recorded behind the last such chain.  A block is reused (or freed)
    // only when no InstRef holds it and those events have completed.
    struct InstBlock {
        float *d = nullptr;      // the entries: `stride` floats each
        uint64_t cap = 0;        // floats the block holds
        uint32_t stride = tr::INST_FLOATS;  // floats per entry: INST_FLOATS {offset xyz, scale} or INST_XFORM_FLOATS (a transform table)
        hipEvent_t used[3] = {}; // behind the last chain on the main stream, setup_stream, setup_stream2 that read it
    };
    // Morph targets (tr_scene_set_morph_targets / _weights) and skinning (tr_scene_set_skin / _bone_palette).  A pose is
    // the host's copy of a weight vector, of a bone palette, or of both (one with neither is no pose: the pointer is
    // null) and, from the first render that draws it, its posed rows on the device: what DevMesh::tri points at instead
    // of d_tri.  The rows have the lifetime of an instance table's block: written once -- by k_morph and, behind it,
    // k_skin in place, queued ahead of the first chain that
    // reads them (blend_poses) -- and never again while anybody may render with them; the holders are the same (a pose
    // travels in the InstRef beside the table).  When the last holder lets go, the rows go back to the scene's pool
    // (pose_free) with one event per stream whose chains read them; they are handed out again when those have completed.
    struct SharedEvent {
        hipEvent_t ev = nullptr;
        ~SharedEvent() { if (ev) (void)hipEventDestroy(ev); }
    };
    struct PoseRows {
        float *d = nullptr;                     // n_rows * TRI_FLOATS
        std::shared_ptr<SharedEvent> used[3];   // behind the last chain on the main stream, setup_stream, setup_stream2 that read them
    };
    struct Pose {
        tr_scene *owner = nullptr;
        std::vector<float> w;                   // the morph weights: n_targets of them, or none
        std::vector<float> pal;                 // the bone palette: n_bones * INST_XFORM_FLOATS floats, or none
        PoseRows rows;                          // (d null until a render is about to draw the pose: pose_rows)
        bool blended = false;                   // k_morph / k_skin have been queued for the rows
        std::shared_ptr<SharedEvent> done;      // ... and this is recorded behind it, on `done_on`
        hipStream_t done_on = nullptr;
        bool done_seen = false;                 // the host has seen `done` completed: no chain needs to wait for it
        ~Pose();
    };
    struct InstRef {
        std::shared_ptr<InstBlock> blk;  // null: no table (the mesh itself)
        uint32_t off = 0, n = 0;         // entries [off, off + n) of the block
        std::shared_ptr<Pose> pose;      // null: the mesh's own rows
    };
    std::vector<PoseRows> pose_free;     // posed rows nobody holds
    uint32_t pose_rows_live = 0;         // sets of posed rows allocated: held ones and free ones (tr_scene_debug_morph_rows)
    uint32_t n_targets = 0;              // morph targets of the scene
    float *d_delta = nullptr;            // their gathered delta rows: n_targets x n_rows x TRI_FLOATS (uv floats zero, unused)
    std::vector<uint32_t> mesh_idx;      // the mesh's indices (n_rows * 9), kept to gather the targets' deltas
    uint32_t n_pos = 0, n_nrm = 0;
    // k_morph's weights on their way to the device: a ring of page-locked staging buffers and their device copies, one per
    // launch in flight (GROUP_MAX frames x TR_MORPH_MAX_TARGETS floats each); `done` = the launch that last read it
    struct MorphStage {
        float *h = nullptr, *d = nullptr;
        std::shared_ptr<SharedEvent> done;
    } morph_stage[4];
    uint64_t morph_launches = 0;
    uint32_t n_bones = 0;                // bones of the scene's skin (0: no skin)
    uint32_t *d_skin = nullptr;          // its gathered influence rows: n_rows x SKIN_ROW_WORDS
    // k_skin's palettes on their way to the device: the same ring (GROUP_MAX frames x TR_SKIN_MAX_BONES entries each)
    MorphStage skin_stage[4];
    uint64_t skin_launches = 0;
    InstRef inst;                    // the current table
    std::vector<std::shared_ptr<InstBlock>> inst_blocks;  // every block the scene owns
    uint32_t n_rows = 0;             // polygons of the mesh (rows of d_tri)
    uint64_t poly_cap = 0;           // polygons of a pass the per-pass record arrays hold
    bool auto_bin_cap = true;        // tr_options.bin_capacity was 0: the pools follow the polygon count
    DevFrame frame = {};       // the rows this scene owns (colour passes)
    DevFrame frame_full = {};  // the whole frame: depth passes fill the entire shadow buffer, whose
                               // lookups are in light space and can land anywhere (shader.rs:774-778)
    uint32_t n_tiles = 0, n_tiles_full = 0;

    // device allocations
    float *d_tri = nullptr;
    uint32_t *d_texel[4] = { nullptr, nullptr, nullptr, nullptr };
    uint32_t *d_packed = nullptr;  // the colour closure's images as one interleaved, tiled array (tr_texels.h)
    size_t packed_count = 0;       // its words
    int set_fs = 0;                // the closure the set was packed for (the last pass's)
    // Dynamic textures (tr_scene_set_texture*): k_pack_texels rewrites d_texel[which] and the set's words in place on the
    // main stream, behind every tile kernel issued so far; `ev_tex` is recorded behind it and both setup streams wait
    // for it, so that a later chain's k_lit reads the new set.  The host form's images wait in device staging buffers
    // (uploaded on a stream of their own, so that the copy does not queue behind the renders); a buffer is used again
    // when the event behind its launch has completed.
    hipEvent_t ev_tex = nullptr;
    hipStream_t upload_stream = nullptr;
    struct TexStage {
        uint8_t *d = nullptr;
        size_t bytes = 0;
        hipEvent_t done = nullptr;
    };
    std::vector<TexStage> tex_stage;
    // The frame's lit texel image (k_lit, tr_kernels.hip): the normal-map / specular closure once per texel and frame
    // instead of once per fragment, where a frame has many more pixels than the images have texels.
    bool lit = false;
    uint32_t lit_words = 0, lit_bpr = 0, set_bpr = 0;  // words of one lit image; blocks per row of it / of the texel set
    uint32_t *d_lit[LOOKAHEAD] = {};                   // per pass in flight (per-frame path); a group set has its own
    // Per-tile polygon counters (followed by k_order's 16 words).  Colour passes (the scene's band)
    // and depth passes (always the whole frame) have different tile grids, hence a state each.
    // SETS sets: the tile kernel of pass q zeroes set (q + SETS - 1) % SETS, which no pass before
    // q + SETS - 1 touches; meanwhile the setup kernels of passes q + 1 .. q + LOOKAHEAD - 1 (running
    // ahead on the setup stream) fill their own sets.
    struct BinState {
        uint32_t *count[SETS] = {};
        uint64_t seq = 0;           // passes of this kind issued so far
    } bin_color, bin_depth;
    // Record bins and work lists, LOOKAHEAD-buffered by global pass number: pass p's setup fills
    // bins[p % LOOKAHEAD] while the tile kernels of the passes before it may still be reading theirs.
    WorkItem *d_order[LOOKAHEAD] = {};  // the tile kernel's work list (k_order)
    Piece *d_bins[LOOKAHEAD] = {};      // the passes' pools: pool_cap records of rec_pieces x 16 B each
    Piece *d_recs[LOOKAHEAD] = {};      // every polygon's record, once per pass (k_setup -> k_bin)
    // Pass pipelining: the chain of pass p (launch_chain: k_lit, k_setup, k_order, k_bin) runs on `setup_stream`, ordered after the tile
    // kernel of pass p - LOOKAHEAD (which freed its bins and zeroed its counters) and before the tile
    // kernel of pass p on the main stream.  They need only frame constants, so they overlap the tile
    // kernels of earlier passes: consecutive frames are in flight together, like any renderer's.
    hipStream_t setup_stream = nullptr;
    // A second one for the per-frame path: the chains of consecutive passes alternate between the two, so that the chain
    // of pass p + 1 (three dependent kernels, as long as the tile kernel it has to hide behind) starts beside the chain
    // of pass p instead of behind it.  Passes share nothing but the targets the tile kernels write (main stream, in order).
    hipStream_t setup_stream2 = nullptr;
    bool two_setup_streams = true;
    hipEvent_t ev_setup[RING] = {};
    hipEvent_t ev_tile[RING] = {};
    // tr_scene_composite orders two scenes' streams: as src, `ev_comp_ready` is recorded behind the frame on this scene's
    // stream and dst's stream waits for it; as dst, `ev_comp_done` is recorded behind k_composite and src's stream waits
    // for it (created at the first such call; each scene records only its own, so destroying one leaves the other's alone)
    hipEvent_t ev_comp_ready = nullptr, ev_comp_done = nullptr;
    uint64_t pass_seq = 0;
    struct PendingTile {
        int fs, tile_waves, shared, kernel_id;
        uint32_t n_poly = 0;        // polygons of the pass
        bool fused_single = false;  // the pass starts from cleared targets without a winner tap: the fused launches' kernels (launch_tile)
        uint64_t p_seq;
        TileArgs args;
    };
    std::vector<PendingTile> pending;  // passes whose setup is queued and whose tile kernel is not yet
    uint64_t tiles_submitted = 0;      // tile kernels handed to the main stream so far
    // did the newest fused tile launches (every pass of a group, or a fused_single pass) run the interior form of their
    // kernels (tile_launch_is_interior, tr_kernels.h)?  -1: no fused launch yet (tr_scene_interior_tiles)
    int fused_interior = -1;
    uint64_t last_submitted_seq = 0;   // pass number of the newest of them (its ev_tile tells whether the stream is idle)
    uint32_t tile_waves = 0;     // tr_options.tile_waves: 4, 8, 16 or 0 = by tile count
    uint32_t tile_mode = 0;      // tr_options.tile_mode: 1 columns, 2 shared bin, 0 = automatic
    uint32_t pool_cap = 0;       // records in a pass's pool (all its (polygon, tile) pairs); grown should a pass exceed it
    uint32_t rec_pieces = 0;
    uint32_t *d_bin_need = nullptr;
    // First pass (global pass number) whose bins overflowed since the last sync, written by k_setup
    // with an atomic minimum; ~0 = none.  Frames older than the last one cannot be rendered again,
    // so sync compares it with `observed_seq`: passes below that number have been handed to a
    // consumer the library cannot call back (an asynchronous read-back, or a caller's stream).
    unsigned long long *d_overflow_seq = nullptr;
    uint64_t observed_seq = 0;
    // Passes below this number rendered frames into caller-provided buffers that the library can no longer
    // render again (older frames of a tr_scene_render_frames call, frames of an automatic group before its last):
    // a bin overflow among them is reported, like one in a frame that was handed on
    uint64_t unreplayable_seq = 0;
    // The current targets (aliases: the memory belongs to the frame slots below, or to the caller)
    float *d_z = nullptr, *d_shadow = nullptr;
    uint32_t *d_sclean = nullptr;  // the shadow buffer's fast-clear flags (n_tiles_full)
    uint8_t *d_fb = nullptr;      // where the next render writes
    // Frame slots: complete sets of render targets.  Slot 0 is what the scene is created with; the others
    // appear with the first tr_scene_render_frames, whose frame i goes to slot i % (frames per group).
    // `fb` is the library's own colour buffer of the slot (allocated when first needed: callers may
    // bring their own); slots of pipelines without a depth pass share slot 0's shadow buffer.
    struct FrameSlot {
        float *z = nullptr;
        uint32_t *zclean = nullptr;
        float *shadow = nullptr;
        uint32_t *sclean = nullptr;
        uint8_t *fb = nullptr;
        // Transient depth: the slot's frame was rendered from cleared targets with its depth left on the chip
        // (TileArgs::store): z memory and fast-clear flags say nothing; the frame's z is what `z_params` renders.
        // ensure_depth() repeats the colour pass for the depth alone when somebody wants the z buffer.
        bool z_deferred = false;
        tr_frame_params z_params = {};
        InstRef z_inst;  // ... and the instance table it was rendered with
        // The shadow matrix (shader.rs:234-255) the slot's shadow buffer was last rendered under -- or took over with a
        // merged buffer: what tr_scene_shadow_merge compares and tr_scene_render_colour_pass looks the buffer up with
        float shadow_matrix[16] = {};
        bool shadow_matrix_set = false;
    };
    std::vector<FrameSlot> slots;
    int cur_slot = 0;
    uint32_t frames_per_launch = 0;  // tr_options.frames_per_launch; 0 = by tile count
    uint32_t max_slots = 0;          // tr_options.max_frame_slots; 0 = automatic
    bool transient_depth = true;     // a cleared frame's colour pass leaves its depth on the chip (TR_OPT_STORE_DEPTH / TR_DEFER_Z=0: off)
    bool no_long_runs = false;       // the large groups' resources did not fit the device once: the usual groups from then on
    bool broken = false;             // a tile kernel could not be launched behind its chain: counters and ranges are stale
    // One group in flight: bins, counters, work lists and argument tables of its frames' passes
    struct GroupSet {
        Piece *bins = nullptr;      // [pass][frame] x pool_cap records
        Piece *recs = nullptr;      // [pass][frame] x polygons
        uint32_t *count = nullptr;  // [pass][frame] x (n_tiles_full + 16)
        WorkItem *order = nullptr;  // [pass][frame] x n_tiles_full
        uint8_t *d_tables = nullptr, *h_tables = nullptr;  // [pass] x frames SetupArgs, then [pass] x frames TileArgs
        hipEvent_t ev_setup = nullptr, ev_tile = nullptr;
        bool in_flight = false;
        uint32_t pool_cap = 0, frames = 0;  // what the set was allocated for
        uint32_t g = 0;                    // frames of the group it holds now
        uint32_t n_poly = 0;               // polygons of its largest frame (frames may draw different instance tables)
        int tile_waves[2] = { 4, 4 }, shared[2] = { 0, 0 };  // the tile kernels' layout, per pass (decided with the setup)
        bool chain_on_main = false;        // its setup was queued on the main stream itself (nothing was in flight)
        uint32_t *lit = nullptr;           // [frame] x lit_words: the frames' lit texel images (scenes with the lit path)
        // [pass][frame] x 8 words, page-locked and mapped: the list lengths of the passes this set last held
        // (k_bin_group writes them; group_units sizes later tile kernels' grids by them)
        volatile uint32_t *h_lens = nullptr;
        uint32_t *d_lens = nullptr;
    } grp[GROUP_SETS];
    uint64_t group_seq = 0;       // groups whose setup has been queued
    uint64_t group_submitted = 0; // groups whose tile kernels have been queued (<= group_seq)
    bool groups_unfenced = false; // group tile kernels were queued since the setup stream was last ordered behind them
    bool quiescent = false;       // the host has waited for the main stream and queued nothing since
    // Automatic frame groups: cleared frames rendered through the per-frame calls on the library's own stream
    // are held back until a group is full (or anything needs them) and then rendered by fused launches.
    struct DeferredFrame {
        tr_frame_params p;
        uint8_t *fb;  // the colour target that was current at its render()
        InstRef inst; // the instance table that was current at its render()
    };
    std::vector<DeferredFrame> deferred;
    bool auto_group = true;
    uint32_t auto_streak = 0;  // groups that filled up inside a running loop since anything else needed the frames
    // The frames of the last tr_scene_render_frames call that still exist (the last `frames per group` of
    // them): what tr_scene_select_frame chooses from, and what is rendered again after a bin overflow.
    struct {
        std::vector<tr_frame_params> params;
        std::vector<void *> fbs;  // the caller's buffers, or empty
        std::vector<int> slot;
        std::vector<InstRef> inst;  // their instance tables
        uint64_t first_seq = 0;   // pass number of the first of them
    } tail;
    bool last_was_group = false;
    uint8_t *d_view = nullptr;  // scratch for get_z_buffer / get_shadow_buffer
    uint8_t *d_resolved = nullptr;  // tr_scene_get_resolved's / tr_scene_get_accumulated's device buffer, of the largest size asked for so far
    size_t resolved_bytes = 0;
    // tr_scene_depth_of_field and tr_scene_bloom in place: the frame and the flags k_dof / k_bloom write before both are copied over the current
    // frame's (3 * W * H bytes, n_tiles words; allocated at the first such call)
    uint8_t *d_dof_fb = nullptr;
    uint32_t *d_dof_clean = nullptr;
    // tr_scene_set_lut: the colour lookup table as k_grade reads it -- lut_n^3 packed entries, padded to whole 16-byte
    // pieces; lut_c0: its entry 0, what a cleared tile becomes.  lut_n == 0: no table
    uint32_t *d_lut = nullptr;
    uint32_t lut_n = 0, lut_c0 = 0;
    // tr_scene_set_ramp: the depth ramp's table as k_ramp reads it -- ramp_n packed rgba entries, padded to whole 16-byte
    // pieces.  ramp_n == 0: no table.  tr_scene_debug_ramp_grid: the cap and the last grid, as for k_grade
    uint32_t *d_ramp = nullptr;
    uint32_t ramp_n = 0, ramp_cap = 0, ramp_grid = 0;
    // tr_scene_debug_projector_launches: the k_projector launches of this scene so far
    uint32_t projector_launches = 0;
    // tr_scene_debug_relight_launches: the k_relight launches of this scene so far
    uint32_t relight_launches = 0;
    // the distance field's scratch, allocated by the first call that needs it and kept: the mask (a bit a pixel, 64-bit
    // words, rows padded to whole words), the row distances (a byte a pixel), the summary (a byte a word of the mask) and,
    // for the ramp calls alone, the u16 field
    uint64_t *d_dist_mask = nullptr;
    uint8_t *d_dist_h = nullptr, *d_dist_summary = nullptr;
    uint16_t *d_dist_field = nullptr;
    // tr_scene_set_lines: the table and its bins in ONE device block of words, so that it changes hands at once -- the
    // lines_n segments (8 words each), n_tiles + 1 list offsets, the lines_listed non-empty tiles, the lines_entries
    // list entries, in this order.  lines_n == 0: no table
    uint32_t *d_lines = nullptr;
    uint32_t lines_n = 0, lines_listed = 0;
    uint64_t lines_entries = 0;
    // tr_scene_resize: the two axes' tables of the last (width, height, filter) asked for (width == 0: none) in one device
    // block `d`, the page-locked block `h` they are uploaded from and the event behind the last upload (resize_tables);
    // shape, y_span and x_span: what launch_resize wants to know of them
    struct ResizeTables {
        uint8_t *d = nullptr, *h = nullptr;
        hipEvent_t uploaded = nullptr;
        uint32_t width = 0, height = 0, filter = 0;
        ResizeTable x = {}, y = {};
        int shape = -1;
        uint32_t y_span = 0, x_span = 0;
    } resize;
    // tr_scene_set_warp: the node grids of the last call (width == 0: none) in the device block `d`, the page-locked block
    // `h` they are uploaded from -- both grown on demand, `cap` int32 each -- and the event behind the last upload
    struct WarpGrid {
        int32_t *d = nullptr, *h = nullptr;
        size_t cap = 0;
        hipEvent_t uploaded = nullptr;
        uint32_t width = 0, height = 0, n_grids = 0;
    } warp;
    // tr_scene_debug_grade_grid: the most workgroups a k_grade launch may start (0: no cap) and what the last one started
    uint32_t grade_cap = 0, grade_grid = 0;
    // tr_scene_frame_stats: the slots k_stats' workgroups store their partial records to (stats_slots of them, allocated
    // at the first call), and tr_scene_debug_stats_grid's cap and last grid, as for k_grade
    uint32_t *d_stats_partials = nullptr;
    uint32_t stats_slots = 0, stats_cap = 0, stats_grid = 0;
    uint32_t *d_winner = nullptr;
    // Fast depth clear: one word per colour-pass tile, non-zero = "every z of the tile is f32::MIN,
    // memory not written".  Raised by the tile kernel for the empty tiles of a cleared frame (and by
    // a clear that has to be materialised), lowered by whoever writes the tile's z.
    uint32_t *d_zclean = nullptr;
    // Colour counterpart, one flag set per frame buffer the scene has rendered into (its own, and the
    // ones a caller alternates through tr_scene_set_frame_buffer_device): non-zero = the tile's colour
    // and winner words in THAT buffer hold the cleared value, so an empty tile of a cleared frame is
    // not stored again.  The buffer belongs to the scene while it is the target: whoever else writes
    // its rows must call tr_scene_set_frame_buffer_device again (which forgets the flags of a buffer
    // it has not seen, and keeps those of one it has).
    struct FbFlags {
        uint8_t *fb;
        uint32_t *clean;
    };
    std::vector<FbFlags> fb_flags;
    uint32_t *d_fbclean = nullptr;  // the current target's set
    // Sparse read-back (tr_scene_get_frame_buffer_async into tr_host_alloc memory): per host buffer, which tiles of it
    // hold zeros since this scene last wrote them there (device memory, updated by k_read_back)
    struct HostFlags {
        void *host;
        uint64_t serial;
        uint32_t *clean;
        uint64_t gen;  // HostAlloc::gen as this scene's last read-back into the buffer left it
    };
    std::vector<HostFlags> host_flags;
    uint64_t *d_stamps = nullptr;
    uint32_t *d_err = nullptr;
    // page-locked host word the kernels set beside d_err (TileArgs::alarm), and its device address
    volatile uint32_t *h_alarm = nullptr;
    uint32_t *d_alarm = nullptr;

    // Lazy clear (scene.rs:128-137): `clear` only records that the targets are logically
    // f32::MIN / 0; the next render writes every pixel of them anyway, and a getter that comes
    // first materialises the values.
    bool z_fb_cleared = false;    // z buffer, frame buffer (and winner tap) are logically cleared
    bool shadow_cleared = false;  // shadow buffer is logically cleared

    tr_uniforms uniforms = {};
    int host_status = TR_OK;  // sticky failure of the last render's host-side prepare

    // What the last render() started from, so that a frame whose bins overflowed can be
    // rendered again after the bins have grown.
    struct {
        tr_frame_params view;
        bool z_fb_cleared, shadow_cleared;
        bool valid;
        InstRef inst;
    } last;

    bool profiling = false;
    std::vector<EventPair> events;
    std::vector<hipEvent_t> event_pool;
    double prof_ms[K_COUNT] = {};
    uint64_t prof_n[K_COUNT] = {};
    uint64_t prof_frames[K_COUNT] = {};
    std::vector<float> frame_intervals_us;  // completion-to-completion time of consecutive colour-pass tile kernels
};

// The last holder of a pose lets go: its rows go back to the scene's pool with the events of their readers.
tr_scene::Pose::~Pose()
{
    if (rows.d && owner) owner->pose_free.push_back(rows);
}

namespace {

template <typename T>
int dev_alloc(T **p, size_t count)
{
    const hipError_t e = hipMalloc(reinterpret_cast<void **>(p), (count ? count : 1) * sizeof(T));
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();  // (not sticky: the caller may go on with less)
        *p = nullptr;
        char buf[96];
        snprintf(buf, sizeof buf, "out of device memory (%zu bytes)", (count ? count : 1) * sizeof(T));
        return tr::fail(TR_E_NOMEM, buf);
    }
    HIP_TRY(e);
    return TR_OK;
}

template <typename T>
void dev_free(T *&p)
{
    if (p) (void)hipFree(p);
    p = nullptr;
}

// The flag set of frame buffer `fb` (allocated zeroed = "content unknown" the first time a buffer is seen;
// a few dozen buffers are remembered: a caller's double-buffered groups of frames, the scene's own slots).
int fb_flags_for(tr_scene *s, uint8_t *fb, uint32_t **out, bool forget = false)
{
    for (const tr_scene::FbFlags &f : s->fb_flags)
        if (f.fb == fb) {
            // `forget`: a caller's buffer handed over again without TR_OPT_TRUST_FRAME_BUFFERS -- anybody may have
            // written it since: "content unknown" (on the main stream: after the tile kernels that used the flags)
            if (forget) HIP_TRY(hipMemsetAsync(f.clean, 0, (size_t)s->n_tiles * 4, s->stream));
            *out = f.clean;
            return TR_OK;
        }
    if (s->fb_flags.size() >= 4u * GROUP_MAX + 8u) {  // forget the oldest that is not the current target's
        (void)hipStreamSynchronize(s->stream);
        size_t k = 0;
        while (k + 1 < s->fb_flags.size() && s->fb_flags[k].clean == s->d_fbclean) k++;
        dev_free(s->fb_flags[k].clean);
        s->fb_flags.erase(s->fb_flags.begin() + (long)k);
    }
    tr_scene::FbFlags f = { fb, nullptr };
    int st = dev_alloc(&f.clean, (size_t)s->n_tiles);
    if (st != TR_OK) return st;
    HIP_TRY(hipMemsetAsync(f.clean, 0, (size_t)s->n_tiles * 4, s->stream));
    s->fb_flags.push_back(f);
    *out = f.clean;
    return TR_OK;
}

// Is `fb` one of the scene's own colour buffers (whose remembered flags always hold)?
bool own_frame_buffer(const tr_scene *s, const uint8_t *fb)
{
    for (const tr_scene::FrameSlot &fs : s->slots)
        if (fs.fb == fb) return true;
    return false;
}

int select_fb_flags(tr_scene *s, bool handed_over = false)
{
    uint32_t *clean = nullptr;
    const bool forget = handed_over && !(s->flags & TR_OPT_TRUST_FRAME_BUFFERS) && !own_frame_buffer(s, s->d_fb);
    int st = fb_flags_for(s, s->d_fb, &clean, forget);
    if (st != TR_OK) return st;
    // the winner tap is one buffer shared by all targets: its tiles were last written with another
    // target's frame, so a remembered "clean" says nothing about them
    if (s->d_winner && s->d_fbclean != clean) HIP_TRY(hipMemsetAsync(clean, 0, (size_t)s->n_tiles * 4, s->stream));
    s->d_fbclean = clean;
    return TR_OK;
}

// The library's own colour buffer of a slot, zero-filled when it is created (Scene::new, scene.rs:71).
int slot_own_fb(tr_scene *s, int k, uint8_t **out)
{
    tr_scene::FrameSlot &fs = s->slots[(size_t)k];
    if (!fs.fb) {
        const size_t n = (size_t)s->width * s->height * 3;
        int st = dev_alloc(&fs.fb, n);
        if (st != TR_OK) return st;
        HIP_TRY(hipMemsetAsync(fs.fb, 0, n, s->stream));
        uint32_t *clean = nullptr;
        st = fb_flags_for(s, fs.fb, &clean);
        if (st != TR_OK) return st;
        if (!s->d_winner) HIP_TRY(hipMemsetAsync(clean, 0xFF, (size_t)s->n_tiles * 4, s->stream));  // zeros = the cleared colour
    }
    *out = fs.fb;
    return TR_OK;
}

// Makes slot k the current set of targets; colour goes to `fb` (a caller's buffer) or, if null, to the
// slot's own buffer.
int use_slot(tr_scene *s, int k, uint8_t *fb, bool handed_over = false)
{
    const tr_scene::FrameSlot &fs = s->slots[(size_t)k];
    s->cur_slot = k;
    s->d_z = fs.z;
    s->d_zclean = fs.zclean;
    s->d_shadow = fs.shadow;
    s->d_sclean = fs.sclean;
    if (!fb) {
        int st = slot_own_fb(s, k, &fb);
        if (st != TR_OK) return st;
    }
    s->d_fb = fb;
    return select_fb_flags(s, handed_over);
}

// The z buffer of frame slot k, allocated the first time a pass will read or write it.  The slots of frame groups
// (ensure_slots) start without one: a cleared frame's colour pass leaves its depth on the chip (transient depth), so a
// slot's z memory is touched only by a depth-only repeat (ensure_depth), an accumulating render or a scene that stores
// its depth -- 64 MiB per slot at 4096^2 that a running loop never uses (32 slots: 2 of the scene's 5 GB).
int need_z(tr_scene *s, int k)
{
    tr_scene::FrameSlot &fs = s->slots[(size_t)k];
    if (!fs.z) {
        int st = dev_alloc(&fs.z, (size_t)s->width * s->height);
        if (st != TR_OK) return st;
    }
    if (k == s->cur_slot) s->d_z = fs.z;
    return TR_OK;
}

// ---------------------------------------------------------------------------------------------
// Instance tables
// ---------------------------------------------------------------------------------------------

// What a pass drawing under table `r` reads (DevMesh, tr_types.h).
DevMesh mesh_of(const tr_scene *s, const tr_scene::InstRef &r)
{
    DevMesh m = {};
    m.tri = r.pose ? r.pose->rows.d : s->d_tri;  // (a pose's rows: null until pose_rows has run -- run_pass / run_group check)
    m.n_tri = s->n_rows;
    if (r.n) {
        m.inst = r.blk->d + (size_t)r.blk->stride * r.off;
        m.inst_xform = r.blk->stride == (uint32_t)INST_XFORM_FLOATS ? 1u : 0u;
        m.n_rows = s->n_rows;
        m.n_tri = s->n_rows * r.n;  // (below 0xFFFFFFF0: checked by set_instances)
    }
    return m;
}

// Makes `r` the scene's current table.
void use_inst(tr_scene *s, const tr_scene::InstRef &r)
{
    s->inst = r;
    s->mesh = mesh_of(s, r);
}

// What the scene draws now -- the view and the table / pose -- held while the library renders a frame of its own accord
// under that frame's state (a replay, a depth-only repeat, a frame held back, a group), and put back when the scope
// ends, whichever way it ends.  Allocates nothing: tr_scene_render -> flush_deferred runs every step of a loop.
struct DrawState {
    tr_scene *const s;
    const tr_frame_params view;
    const tr_scene::InstRef inst;
    explicit DrawState(tr_scene *scene) : s(scene), view(scene->view), inst(scene->inst) {}
    ~DrawState()
    {
        s->view = view;
        use_inst(s, inst);
    }
    DrawState(const DrawState &) = delete;
    DrawState &operator=(const DrawState &) = delete;
};

// A chain that reads table `m` (a DevMesh of mesh_of) has been queued on `st`: the block may not be written or freed
// until what is queued there now has run.  (No table: nothing to do -- the scene without instances queues nothing more.)
int note_inst_use(tr_scene *s, const DevMesh &m, hipStream_t st)
{
    if (!m.inst) return TR_OK;
    const int k = st == s->setup_stream ? 1 : st == s->setup_stream2 ? 2 : 0;
    for (const std::shared_ptr<tr_scene::InstBlock> &b : s->inst_blocks)
        if (m.inst >= b->d && m.inst < b->d + b->cap) {
            if (!b->used[k]) HIP_TRY(hipEventCreateWithFlags(&b->used[k], hipEventDisableTiming));
            HIP_TRY(hipEventRecord(b->used[k], st));
            return TR_OK;
        }
    return tr::fail(TR_E_INVALID, "instance table not owned by the scene");
}

void free_inst_block(tr_scene::InstBlock &b)
{
    for (hipEvent_t &e : b.used) {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
    if (b.d) (void)hipFree(b.d);
    b.d = nullptr;
    b.cap = 0;
}

// Waits for the chains that read block `b` (a block nobody holds any more: no new ones can be queued).
int inst_block_idle(tr_scene::InstBlock &b)
{
    for (hipEvent_t e : b.used)
        if (e) HIP_TRY(hipEventSynchronize(e));
    return TR_OK;
}

// Copies `n` entries of `h`, `stride` floats each (the table's kind), into a block of their own: one nobody holds whose
// readers have run, else a new one.
int upload_instances(tr_scene *s, uint32_t n, uint32_t stride, const float *h, tr_scene::InstRef &out)
{
    const uint64_t floats = (uint64_t)n * stride;
    std::shared_ptr<tr_scene::InstBlock> pick;
    // free blocks: prefer one whose readers have finished; a free block too small for the table is given back
    for (size_t i = 0; i < s->inst_blocks.size();) {
        std::shared_ptr<tr_scene::InstBlock> &b = s->inst_blocks[i];
        if (b.use_count() > 1) {
            i++;
            continue;
        }
        if (b->cap < floats) {
            int st = inst_block_idle(*b);
            if (st != TR_OK) return st;
            free_inst_block(*b);
            s->inst_blocks.erase(s->inst_blocks.begin() + (long)i);
            continue;
        }
        bool done = true;
        for (hipEvent_t e : b->used) done = done && (!e || hipEventQuery(e) == hipSuccess);
        if (!pick || done) pick = b;
        if (done) break;
        i++;
    }
    if (pick) {
        int st = inst_block_idle(*pick);  // (usually long done)
        if (st != TR_OK) return st;
    } else {
        pick = std::make_shared<tr_scene::InstBlock>();
        int st = dev_alloc(&pick->d, (size_t)floats);
        if (st != TR_OK) return st;
        pick->cap = floats;
        s->inst_blocks.push_back(pick);
    }
    pick->stride = stride;
    HIP_TRY(hipMemcpy(pick->d, h, sizeof(float) * (size_t)floats, hipMemcpyHostToDevice));
    HIP_TRY(hipStreamSynchronize(nullptr));  // (the scene's streams do not wait for the null stream)
    out.blk = pick;
    out.off = 0;
    out.n = n;
    return TR_OK;
}

// ---------------------------------------------------------------------------------------------
// Morph targets
// ---------------------------------------------------------------------------------------------

hipEvent_t take_event(tr_scene *s);
int launch_status(int rc, const char *what);

std::shared_ptr<tr_scene::SharedEvent> new_shared_event()
{
    std::shared_ptr<tr_scene::SharedEvent> e = std::make_shared<tr_scene::SharedEvent>();
    if (hipEventCreateWithFlags(&e->ev, hipEventDisableTiming) != hipSuccess) {
        e->ev = nullptr;
        return nullptr;
    }
    return e;
}

// A pose of the scene's targets under weights w[0 .. n_targets) (null: no weights) and of its skin under the palette
// pal[0 .. n_bones * INST_XFORM_FLOATS) (null: no palette); neither: no pose.
std::shared_ptr<tr_scene::Pose> make_pose(tr_scene *s, const float *w, const float *pal)
{
    if (!w && !pal) return nullptr;
    std::shared_ptr<tr_scene::Pose> p = std::make_shared<tr_scene::Pose>();
    p->owner = s;
    if (w) p->w.assign(w, w + s->n_targets);
    if (pal) p->pal.assign(pal, pal + (size_t)s->n_bones * INST_XFORM_FLOATS);
    return p;
}

// The halves of pose `p` (null: none) as make_pose takes them.  A half made under targets or a skin the scene has since
// replaced (a kept frame's, selected again) is not carried over into a new pose: null.
const float *pose_weights(const tr_scene *s, const std::shared_ptr<tr_scene::Pose> &p)
{
    return p && !p->w.empty() && p->w.size() == (size_t)s->n_targets ? p->w.data() : nullptr;
}
const float *pose_palette(const tr_scene *s, const std::shared_ptr<tr_scene::Pose> &p)
{
    return p && !p->pal.empty() && p->pal.size() == (size_t)s->n_bones * INST_XFORM_FLOATS ? p->pal.data() : nullptr;
}

// Free rows beyond this many are given back to the device (trim_pose_pool): a group's worth may wait for their readers
// while the next group takes its own.
constexpr size_t POSE_FREE_MAX = GROUP_MAX;

bool pose_rows_idle(const tr_scene::PoseRows &r)
{
    for (const std::shared_ptr<tr_scene::SharedEvent> &e : r.used)
        if (e && hipEventQuery(e->ev) != hipSuccess) return false;
    return true;
}

// Gives free rows whose readers have run back to the device until at most `keep` free sets are left (or the rest are
// still being read).
void trim_pose_pool(tr_scene *s, size_t keep)
{
    for (size_t i = 0; i < s->pose_free.size() && s->pose_free.size() > keep;) {
        if (!pose_rows_idle(s->pose_free[i])) {
            i++;
            continue;
        }
        dev_free(s->pose_free[i].d);
        s->pose_free.erase(s->pose_free.begin() + (long)i);
        s->pose_rows_live--;
    }
}

// Device memory for the pose's rows: rows nobody holds whose readers have run, else new ones.  A pose's holders are its
// frame's slot, the kept frames, held-back frames and the current state -- tr_scene_render_frames_morphed makes its poses
// group by group -- so the sets alive are bounded by the frame slots plus the groups in flight, not by the frames of a call.
int pose_rows(tr_scene *s, tr_scene::Pose &p)
{
    if (p.rows.d) return TR_OK;
    size_t pick = s->pose_free.size();
    for (size_t i = 0; i < s->pose_free.size() && pick == s->pose_free.size(); i++)
        if (pose_rows_idle(s->pose_free[i])) pick = i;
    if (pick == s->pose_free.size() && s->pose_free.size() >= POSE_FREE_MAX) {
        pick = 0;  // enough of them wait for their readers: the host waits for the oldest instead of allocating more
        for (const std::shared_ptr<tr_scene::SharedEvent> &e : s->pose_free[0].used)
            if (e) HIP_TRY(hipEventSynchronize(e->ev));
    }
    if (pick < s->pose_free.size()) {
        p.rows.d = s->pose_free[pick].d;
        s->pose_free.erase(s->pose_free.begin() + (long)pick);
        if (s->pose_free.size() > POSE_FREE_MAX) trim_pose_pool(s, POSE_FREE_MAX);
        return TR_OK;
    }
    int st = dev_alloc(&p.rows.d, (size_t)s->n_rows * TRI_FLOATS);
    if (st == TR_OK) s->pose_rows_live++;
    return st;
}

// Chains that read the rows of `poses` (null entries: none) have been queued on `st`: one event behind them, shared by
// the poses, guards the rows' reuse.
int note_pose_use(tr_scene *s, const std::shared_ptr<tr_scene::Pose> *poses, uint32_t n, hipStream_t st)
{
    const int k = st == s->setup_stream ? 1 : st == s->setup_stream2 ? 2 : 0;
    std::shared_ptr<tr_scene::SharedEvent> e;
    for (uint32_t j = 0; j < n; j++) {
        if (!poses[j]) continue;
        if (!e) {
            e = new_shared_event();
            if (!e) return tr::fail(TR_E_HIP, "hipEventCreate failed");
            HIP_TRY(hipEventRecord(e->ev, st));
        }
        poses[j]->rows.used[k] = e;
    }
    return TR_OK;
}

// One launch's worth of per-frame vectors (k_morph's weights, k_skin's palettes) through the ring `ring`: slot
// `launches % 4`, allocated on first use for `floats` floats, free again once the launch that last read it has run.
int take_stage(tr_scene::MorphStage *ring, uint64_t launches, size_t floats, tr_scene::MorphStage **out)
{
    tr_scene::MorphStage &stage = ring[launches % 4u];
    int st = TR_OK;
    if (!stage.h) HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&stage.h), sizeof(float) * floats, hipHostMallocDefault));
    if (!stage.d && (st = dev_alloc(&stage.d, floats)) != TR_OK) return st;
    if (stage.done) HIP_TRY(hipEventSynchronize(stage.done->ev));  // (four launches ago: long done)
    *out = &stage;
    return TR_OK;
}

// Before a chain on `chain` reads the rows of `poses` (null entries and repeats allowed): the ones not blended yet get
// their rows; those with weights are blended by ONE launch of k_morph on `chain`, those with a palette are then skinned
// by ONE launch of k_skin behind it (in place where k_morph wrote the rows, from the mesh's own rows otherwise), and one
// event behind the last launch stands for both; the chain waits for those blended on another stream.
int blend_poses(tr_scene *s, const std::shared_ptr<tr_scene::Pose> *poses, uint32_t n, hipStream_t chain)
{
    tr_scene::Pose *todo[GROUP_MAX];
    uint32_t m = 0, m_morph = 0, m_skin = 0;
    for (uint32_t j = 0; j < n; j++) {
        tr_scene::Pose *p = poses[j].get();
        if (!p) continue;
        if (p->blended) {
            if (p->done_on != chain && !p->done_seen) {
                if (hipEventQuery(p->done->ev) == hipSuccess) p->done_seen = true;
                else HIP_TRY(hipStreamWaitEvent(chain, p->done->ev, 0));
            }
            continue;
        }
        bool listed = false;  // (a pose that several frames draw is blended once)
        for (uint32_t i = 0; i < m; i++) listed = listed || todo[i] == p;
        if (listed) continue;
        if (!p->w.empty() && (p->w.size() != (size_t)s->n_targets || !s->d_delta))
            return tr::fail(TR_E_INVALID, "pose of targets the scene no longer has");
        if (!p->pal.empty() && (p->pal.size() != (size_t)s->n_bones * INST_XFORM_FLOATS || !s->d_skin))
            return tr::fail(TR_E_INVALID, "palette of a skin the scene no longer has");
        if (p->w.empty() && p->pal.empty()) return tr::fail(TR_E_INVALID, "empty pose");
        if (m >= (uint32_t)GROUP_MAX) return tr::fail(TR_E_INVALID, "too many poses for one launch");
        int st = pose_rows(s, *p);
        if (st != TR_OK) return st;
        todo[m++] = p;
        m_morph += p->w.empty() ? 0u : 1u;
        m_skin += p->pal.empty() ? 0u : 1u;
    }
    if (m == 0) return TR_OK;
    int st = TR_OK;
    tr_scene::MorphStage *morph_stage = nullptr, *skin_stage = nullptr;
    if (m_morph) {
        const uint32_t T = s->n_targets;
        if ((st = take_stage(s->morph_stage, s->morph_launches, (size_t)GROUP_MAX * TR_MORPH_MAX_TARGETS, &morph_stage)) != TR_OK) return st;
        tr_scene::MorphStage &stage = *morph_stage;
        MorphTable tab = {};
        uint32_t k = 0;
        for (uint32_t j = 0; j < m; j++) {
            if (todo[j]->w.empty()) continue;
            memcpy(stage.h + (size_t)k * T, todo[j]->w.data(), sizeof(float) * T);
            tab.f[k].w = stage.d + (size_t)k * T;
            tab.f[k].dst = todo[j]->rows.d;
            k++;
        }
        HIP_TRY(hipMemcpyAsync(stage.d, stage.h, sizeof(float) * (size_t)k * T, hipMemcpyHostToDevice, chain));
        EventPair ep = { nullptr, nullptr, K_MORPH, k };
        if (s->profiling) { ep.a = take_event(s); ep.b = take_event(s); }
        int rc = launch_morph(s->d_tri, s->d_delta, s->n_rows, T, tab, k, chain, ep.a, ep.b);
        if (rc) return launch_status(rc, "k_morph");
        if (s->profiling) s->events.push_back(ep);
    }
    if (m_skin) {
        const size_t B = (size_t)s->n_bones * INST_XFORM_FLOATS;  // floats of a palette (a multiple of four: 16-byte pieces)
        if ((st = take_stage(s->skin_stage, s->skin_launches, (size_t)GROUP_MAX * TR_SKIN_MAX_BONES * INST_XFORM_FLOATS, &skin_stage)) != TR_OK)
            return st;
        tr_scene::MorphStage &stage = *skin_stage;
        SkinTable tab = {};
        uint32_t k = 0;
        for (uint32_t j = 0; j < m; j++) {
            if (todo[j]->pal.empty()) continue;
            memcpy(stage.h + (size_t)k * B, todo[j]->pal.data(), sizeof(float) * B);
            tab.f[k].pal = stage.d + (size_t)k * B;
            tab.f[k].src = todo[j]->w.empty() ? s->d_tri : todo[j]->rows.d;  // (the morphed rows, in place; else the mesh's own)
            tab.f[k].dst = todo[j]->rows.d;
            k++;
        }
        HIP_TRY(hipMemcpyAsync(stage.d, stage.h, sizeof(float) * (size_t)k * B, hipMemcpyHostToDevice, chain));
        EventPair ep = { nullptr, nullptr, K_SKIN, k };
        if (s->profiling) { ep.a = take_event(s); ep.b = take_event(s); }
        int rc = launch_skin(s->d_skin, s->n_rows, s->n_bones, tab, k, chain, ep.a, ep.b);
        if (rc) return launch_status(rc, "k_skin");
        if (s->profiling) s->events.push_back(ep);
    }
    std::shared_ptr<tr_scene::SharedEvent> done = new_shared_event();
    if (!done) return tr::fail(TR_E_HIP, "hipEventCreate failed");
    HIP_TRY(hipEventRecord(done->ev, chain));
    if (morph_stage) {
        morph_stage->done = done;
        s->morph_launches++;
    }
    if (skin_stage) {
        skin_stage->done = done;
        s->skin_launches++;
    }
    for (uint32_t j = 0; j < m; j++) {
        todo[j]->blended = true;
        todo[j]->done = done;
        todo[j]->done_on = chain;
    }
    return TR_OK;
}

hipEvent_t take_event(tr_scene *s)
{
    if (!s->event_pool.empty()) {
        hipEvent_t e = s->event_pool.back();
        s->event_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}

// A launch's profile record: with its two timing events while the scene is profiling, else with none (the launchers
// take null events); whoever launched pushes it onto s->events when it has events.
EventPair timing_pair(tr_scene *s, int kernel, uint32_t frames)
{
    EventPair ep = { nullptr, nullptr, kernel, frames };
    if (s->profiling) {
        ep.a = take_event(s);
        ep.b = take_event(s);
    }
    return ep;
}

struct Timed {
    tr_scene *s;
    hipStream_t st;
    EventPair ep;
    bool on;
    Timed(tr_scene *sc, int kernel, hipStream_t stream = nullptr) : s(sc), st(stream ? stream : sc->stream), on(false)
    {
        ep.kernel = kernel;
        ep.frames = 1u;
        ep.a = ep.b = nullptr;
        if (s->profiling && s->events.size() < (1u << 20)) {
            ep.a = take_event(s);
            ep.b = take_event(s);
            if (ep.a && ep.b && hipEventRecord(ep.a, st) == hipSuccess) on = true;
        }
    }
    ~Timed()
    {
        if (on && hipEventRecord(ep.b, st) == hipSuccess) s->events.push_back(ep);
    }
};

int drain_events(tr_scene *s)
{
    hipEvent_t prev_frame_end = nullptr;
    for (const EventPair &ep : s->events) {
        float ms = 0.0f;
        if (hipEventSynchronize(ep.b) == hipSuccess && hipEventElapsedTime(&ms, ep.a, ep.b) == hipSuccess) {
            s->prof_ms[ep.kernel] += ms;
            s->prof_n[ep.kernel] += 1;
            s->prof_frames[ep.kernel] += ep.frames;
        }
        if (ep.kernel == K_TILE) {
            // a frame ends with its colour pass: the spacing of those completions is the frame time
            // of the running pipeline (frames overlap; a kernel's own duration says less); a fused
            // launch completes its frames together: each gets an equal share of the spacing
            if (prev_frame_end && hipEventElapsedTime(&ms, prev_frame_end, ep.b) == hipSuccess)
                for (uint32_t k = 0; k < ep.frames && s->frame_intervals_us.size() < (1u << 20); k++)
                    s->frame_intervals_us.push_back(ms * 1000.0f / (float)ep.frames);
            prev_frame_end = ep.b;
        }
        s->event_pool.push_back(ep.a);
        s->event_pool.push_back(ep.b);
    }
    s->events.clear();
    return TR_OK;
}

int launch_status(int rc, const char *what)
{
    if (rc == 0) return TR_OK;
    return tr::fail(TR_E_HIP, std::string(what) + ": " + hipGetErrorString((hipError_t)rc));
}

// Enqueues one pending pass's tile kernel on the main stream.
int launch_pending_tile(tr_scene *s, const tr_scene::PendingTile &t)
{
    int status = TR_OK;
    // (the pass's "tile done" event rides on the kernel's own completion signal; profiling: recorded behind its timing events)
    const EventPair ep = timing_pair(s, t.kernel_id, 1u);
    hipEvent_t tile_done = s->ev_tile[t.p_seq % RING];
    int rc = launch_tile(t.fs, t.args, t.tile_waves, t.shared, t.n_poly, nullptr, 0, s->stream, ep.a, s->profiling ? ep.b : tile_done, 0u,
                         t.fused_single);
    if (rc) status = launch_status(rc, "k_tile");
    if (rc) s->broken = true;  // (its chain has run: the set's counters were not zeroed, the pass's ranges never consumed)
    if (s->profiling) {
        s->events.push_back(ep);
        if (hipEventRecord(tile_done, s->stream) != hipSuccess && status == TR_OK) status = tr::fail(TR_E_HIP, "hipEventRecord");
    }
    if (t.fused_single) s->fused_interior = tile_launch_is_interior(t.fs, t.args, t.tile_waves, t.shared, t.n_poly, true) ? 1 : 0;
    s->tiles_submitted += 1;
    s->last_submitted_seq = t.p_seq;
    return status;
}

// Puts ALL pending per-frame tile kernels on the main stream: one wait for the setup stream (it is in
// order, so the newest pass's event covers the older ones), then the kernels back to back.
int submit_pending_tiles(tr_scene *s)
{
    if (s->pending.empty()) return TR_OK;
    // (each setup stream is in order: its newest pass's event covers the older ones)
    HIP_TRY(hipStreamWaitEvent(s->stream, s->ev_setup[s->pending.back().p_seq % RING], 0));
    if (s->two_setup_streams && s->pending.size() > 1u)
        HIP_TRY(hipStreamWaitEvent(s->stream, s->ev_setup[s->pending[s->pending.size() - 2u].p_seq % RING], 0));
    int status = TR_OK;
    for (const tr_scene::PendingTile &t : s->pending) {
        int st = launch_pending_tile(s, t);
        if (st != TR_OK && status == TR_OK) status = st;
    }
    s->pending.clear();
    return status;
}

// The oldest pending pass alone, behind a wait for its own setup if that may still be running.
int submit_front(tr_scene *s, bool wait_for_setup)
{
    if (s->pending.empty()) return TR_OK;
    const tr_scene::PendingTile t = s->pending.front();
    if (wait_for_setup) HIP_TRY(hipStreamWaitEvent(s->stream, s->ev_setup[t.p_seq % RING], 0));
    s->pending.erase(s->pending.begin());
    return launch_pending_tile(s, t);
}

// Every pending pass whose setup has completed, oldest first, without any cross-stream wait.
int submit_ready(tr_scene *s)
{
    int status = TR_OK;
    while (!s->pending.empty() && hipEventQuery(s->ev_setup[s->pending.front().p_seq % RING]) == hipSuccess) {
        int st = submit_front(s, false);
        if (st != TR_OK && status == TR_OK) status = st;
    }
    return status;
}

int flush_deferred(tr_scene *s, bool hold_back);
int finish_groups(tr_scene *s);

// Everything the scene has been asked to render goes to the device: frames `render` has held back to fuse
// them (below, "Automatic frame groups"), per-frame tile kernels waiting for their setup, groups' tile
// kernels.  Runs before every use of the main stream and before anything waits for the scene.
int submit_pending(tr_scene *s)
{
    int st = flush_deferred(s, false);
    int st2 = submit_pending_tiles(s);
    int st3 = finish_groups(s);
    return st != TR_OK ? st : st2 != TR_OK ? st2 : st3;
}

// Materialise a pending clear of the z / frame buffers (and winner tap).
int flush_clear_color(tr_scene *s)
{
    {
        int sp = submit_pending(s);
        if (sp != TR_OK) return sp;
    }
    if (!s->z_fb_cleared) return TR_OK;
    // only the rows this scene owns: in a band-sharded frame the rest belongs to other ranks
    const size_t W = s->width;
    const size_t n = W * (size_t)(s->frame.band_y1 - s->frame.band_y0);
    const size_t z_first = W * (size_t)s->frame.band_y0;
    const size_t fb_first = W * (size_t)(s->height - (uint32_t)s->frame.band_y1) * 3;
    Timed t(s, K_CLEAR);
    // z: raise every tile's fast-clear flag; colour (and the winner tap) are real memory
    HIP_TRY(hipMemsetAsync(s->d_zclean, 0xFF, (size_t)s->n_tiles * 4, s->stream));
    s->slots[(size_t)s->cur_slot].z_deferred = false;   // (the slot's z IS the cleared value now)
    HIP_TRY(hipMemsetAsync(s->d_fb + fb_first, 0, n * 3, s->stream));
    HIP_TRY(hipMemsetAsync(s->d_fbclean, 0xFF, (size_t)s->n_tiles * 4, s->stream));
    if (s->d_winner) HIP_TRY(hipMemsetAsync(s->d_winner + z_first, 0xFF, n * 4, s->stream));
    s->z_fb_cleared = false;
    return TR_OK;
}

int flush_clear_shadow(tr_scene *s)
{
    if (!s->shadow_cleared) return TR_OK;
    {
        int sp = submit_pending(s);
        if (sp != TR_OK) return sp;
    }
    // a cleared shadow buffer = every tile's fast-clear flag up (lookups consult the flags; getters
    // materialise the values first)
    Timed t(s, K_CLEAR);
    HIP_TRY(hipMemsetAsync(s->d_sclean, 0xFF, (size_t)s->n_tiles_full * 4, s->stream));
    s->shadow_cleared = false;
    return TR_OK;
}

// Gives the shadow buffer plain-memory meaning for a getter.
int materialize_shadow(tr_scene *s)
{
    {
        int sp = submit_pending(s);
        if (sp != TR_OK) return sp;
    }
    int rc = launch_materialize_depth(s->d_shadow, s->d_sclean, s->frame_full, s->stream);
    if (rc) return launch_status(rc, "k_materialize_depth");
    return TR_OK;
}

// Gives the z buffer plain-memory meaning: tiles still behind their fast-clear flag get their f32::MIN.
int materialize_depth(tr_scene *s)
{
    {
        int sp = submit_pending(s);
        if (sp != TR_OK) return sp;
    }
    {
        int st = need_z(s, s->cur_slot);
        if (st != TR_OK) return st;
    }
    int rc = launch_materialize_depth(s->d_z, s->d_zclean, s->frame, s->stream);
    if (rc) return launch_status(rc, "k_materialize_depth");
    return TR_OK;
}

int render_frame(tr_scene *s);
int replay_tail(tr_scene *s);
int ensure_depth(tr_scene *s);

// Tiles the bins must cover: a band scene's colour passes touch its own rows only; the depth passes of
// shadow / occlusion fill the whole shadow buffer on every rank (shader.rs:774-778).

// How the waves of a tile divide the work when tr_options.tile_mode leaves it open (speed only).
int tile_mode_auto(int by_tile_count)
{
    static const int forced = getenv("TR_TILE_MODE") ? atoi(getenv("TR_TILE_MODE")) : 0;  // test hook: 1 columns, 2 shared
    if (forced == 1 || forced == 2) return forced == 2;
    return by_tile_count;
}

// A tile received more polygons than its bin holds (k_tile then works on the first bin_cap records
// only: a truncated frame).  Grow the bins to what the passes asked for, then:
//   * if an overflowed pass has already been handed to a consumer the library cannot call back --
//     an asynchronous read-back queued behind it, or a caller-provided stream, whose next
//     operation may have used the frame -- report TR_E_BIN_OVERFLOW: the caller renders (and
//     copies) again, now with bins that fit;
//   * otherwise only the last frame can still be observed: render it again from the state it
//     started in.  Exact when that frame started from cleared targets (the per-frame protocol of
//     app.rs:170-210); an accumulating render cannot be replayed and reports TR_E_BIN_OVERFLOW.
int recover_from_overflow(tr_scene *s, unsigned long long first_bad_seq)
{
    uint32_t need = 0;
    HIP_TRY(hipMemcpy(&need, s->d_bin_need, sizeof need, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemset(s->d_bin_need, 0, sizeof need));
    HIP_TRY(hipStreamSynchronize(nullptr));  // (the scene's streams do not wait for the null stream)
    const uint64_t cap = plan::grown_pool(s->pool_cap, need);   // (need = the pairs the hungriest pass wanted)
    {
        // per-frame sets + the frame groups' sets, if they exist
        uint64_t sets = LOOKAHEAD;
        for (const tr_scene::GroupSet &g : s->grp) sets += (uint64_t)g.frames * (uint64_t)kPipelines[s->pipeline].n_passes;
        if (cap < need || sets * cap * s->rec_pieces * 16ull > (128ull << 30))
            return tr::fail(TR_E_BIN_OVERFLOW, "the pools of polygon records would exceed 128 GiB");
    }
    HIP_TRY(hipStreamSynchronize(s->setup_stream));
    HIP_TRY(hipStreamSynchronize(s->setup_stream2));
    s->pool_cap = (uint32_t)cap;
    int st = TR_OK;
    for (int k = 0; k < LOOKAHEAD && st == TR_OK; k++) {
        dev_free(s->d_bins[k]);
        st = dev_alloc(&s->d_bins[k], (size_t)s->pool_cap * s->rec_pieces);
    }
    if (st != TR_OK) return st;
    // (the frame groups' bins follow bin_cap when their set is next used)
    // what to do about the frame(s) that were rendered with too small a pool (tr_plan.h, overflow_action)
    const PipelineDesc &pd = kPipelines[s->pipeline];
    plan::OverflowState os;
    os.first_bad_seq = first_bad_seq;
    os.observed_seq = s->observed_seq;
    os.unreplayable_seq = s->unreplayable_seq;
    os.last_was_group = s->last_was_group;
    os.last_valid = s->last.valid;
    os.last_started_cleared = s->last.z_fb_cleared && (pd.n_passes == 1 || s->last.shadow_cleared);
    switch (plan::overflow_action(os)) {
    case plan::OverflowAction::REPORT_CALLERS_BUFFER: {
        char buf[320];
        snprintf(buf, sizeof buf,
                 "triangle bins overflowed in a frame that went to a caller's buffer and cannot be rendered again (an older "
                 "frame of tr_scene_render_frames, or of a fused group of per-frame renders): that buffer holds a truncated "
                 "frame; the pools have been grown to %u records per pass: render it again", s->pool_cap);
        return tr::fail(TR_E_BIN_OVERFLOW, buf);
    }
    case plan::OverflowAction::REPORT_HANDED_ON: {
        char buf[320];
        snprintf(buf, sizeof buf,
                 "triangle bins overflowed in a frame that was already handed on (asynchronous read-back or caller's "
                 "stream): that frame is truncated; the pools have been grown to %u records per pass (a pass wanted %u, "
                 "pass %llu of %llu): render it again", s->pool_cap, need, first_bad_seq, (unsigned long long)s->pass_seq);
        return tr::fail(TR_E_BIN_OVERFLOW, buf);
    }
    case plan::OverflowAction::REPLAY_TAIL:
        return replay_tail(s);  // frames older than the tail no longer exist anywhere
    case plan::OverflowAction::REPORT_ACCUMULATING:
        return tr::fail(TR_E_BIN_OVERFLOW,
                        "triangle bins overflowed during an accumulating render; they have been grown: clear and render again");
    case plan::OverflowAction::REPLAY_LAST:
        break;
    }
    const DrawState now(s);
    s->view = s->last.view;
    use_inst(s, s->last.inst);
    const bool z_now = s->z_fb_cleared, sh_now = s->shadow_cleared;
    s->z_fb_cleared = true;
    s->shadow_cleared = s->last.shadow_cleared;
    st = render_frame(s);
    // a clear() issued after the overflowing render stays pending
    s->z_fb_cleared = s->z_fb_cleared || z_now;
    s->shadow_cleared = s->shadow_cleared || sh_now;
    return st;
}

// Reads and resets the device error word and the overflow bookkeeping (stream idle).
int take_device_errors(tr_scene *s, uint32_t &err, unsigned long long &first_bad_seq)
{
    err = 0;
    first_bad_seq = ~0ull;
    if (*s->h_alarm == 0u) return TR_OK;  // nothing was raised since the last look: no copy
    *s->h_alarm = 0u;
    HIP_TRY(hipMemcpy(&err, s->d_err, sizeof err, hipMemcpyDeviceToHost));
    if (err) {
        HIP_TRY(hipMemset(s->d_err, 0, sizeof err));  // the word is per frame, not sticky
        HIP_TRY(hipStreamSynchronize(nullptr));         // (the scene's streams do not wait for the null stream)
    }
    if (err & DE_BIN_OVERFLOW) {
        HIP_TRY(hipMemcpy(&first_bad_seq, s->d_overflow_seq, sizeof first_bad_seq, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemset(s->d_overflow_seq, 0xFF, sizeof first_bad_seq));
        HIP_TRY(hipStreamSynchronize(nullptr));
    }
    return TR_OK;
}

// Waits for the stream and folds the device error word into a status.
int sync_and_status(tr_scene *s)
{
    HIP_TRY(hipSetDevice(s->device));
    {
        int sp = submit_pending(s);
        if (sp != TR_OK) return sp;
    }
    HIP_TRY(hipStreamSynchronize(s->stream));
    uint32_t err = 0;
    unsigned long long first_bad = ~0ull;
    {
        int st = take_device_errors(s, err, first_bad);
        if (st != TR_OK) return st;
    }
    const int host_status = s->host_status;
    if (err & DE_BIN_OVERFLOW) {
        int st = recover_from_overflow(s, first_bad);
        s->observed_seq = 0;  // everything issued so far has completed; later hand-offs count afresh
        s->unreplayable_seq = 0;
        if (st != TR_OK) return st;
        st = submit_pending(s);
        if (st != TR_OK) return st;
        HIP_TRY(hipStreamSynchronize(s->stream));
        st = take_device_errors(s, err, first_bad);
        if (st != TR_OK) return st;
        if (err & DE_BIN_OVERFLOW) return tr::fail(TR_E_BIN_OVERFLOW, "triangle bins overflowed twice");
    }
    s->observed_seq = 0;
    s->unreplayable_seq = 0;
    s->quiescent = true;  // (whatever a getter queues next -- a view kernel, a copy -- it also waits for)
    if (host_status != TR_OK) return host_status;
    if (err & (DE_W_ZERO | DE_TEX_OOB | DE_SHADOW_OOB | DE_SINGULAR)) {
        char buf[160];
        snprintf(buf, sizeof buf,
                 "device lookups left their range (bits 0x%x: 1 w==0, 2 texture, 4 shadow buffer, 8 singular basis)",
                 err);
        return tr::fail(TR_E_OOB_LOOKUP, buf);
    }
    return TR_OK;
}

void fill_dev_uniforms(const tr_scene *s, DevUniforms &d)
{
    const tr_uniforms &u = s->uniforms;
    memcpy(d.vpmv, u.vpmv, sizeof d.vpmv);
    memcpy(d.m, u.m, sizeof d.m);
    memcpy(d.it_m, u.it_m, sizeof d.it_m);
    memcpy(d.shadow_matrix, u.shadow_matrix, sizeof d.shadow_matrix);
    memcpy(d.i_vpmv, u.i_vpmv, sizeof d.i_vpmv);
    memcpy(d.camera_direction, u.camera_direction, sizeof d.camera_direction);
    memcpy(d.t_light, u.t_light_direction, sizeof d.t_light);
    memset(d.sm_ivpmv, 0, sizeof d.sm_ivpmv);
    memset(d.occl_steps, 0, sizeof d.occl_steps);
}

// The frame constants of one pass (shader.rs:183-279 prepares) for the light and camera the scene holds.
int pass_uniforms(tr_scene *s, const PassDesc &p, DevUniforms &du)
{
    const tr_frame_params &v = s->view;
    int st = prepare_uniforms(p.prepare_kind, &s->uniforms, s->width, s->height, v.light, v.look_from, v.look_at, v.up);
    if (st != TR_OK) return tr::fail(st, "prepare: singular matrix (try_inverse().unwrap() would panic)");
    fill_dev_uniforms(s, du);
    if (p.fs == FS_SHADOW2 || p.fs == FS_OCCLUSION2) shadow_times_inverse(&s->uniforms, du.sm_ivpmv);
    if (p.fs == FS_OCCLUSION2) {
        st = occlusion_steps(&s->uniforms, du.occl_steps);
        if (st != TR_OK) return tr::fail(st, "occlusion: rotation_between(..).unwrap() would panic");
    }
    return TR_OK;
}

// The fragment variant the tile kernel runs for a pass whose closure is `fs`: with the lit path (k_lit) the normal-map
// and specular closures have run per texel, and the fragment stage fetches their result.
int tile_fs(const tr_scene *s, int fs) { return (s->lit && (fs == FS_NORMAL_MAP || fs == FS_SPECULAR)) ? (int)FS_LIT : fs; }

// How a tile's work is divided is a launch-time choice (speed only; tr_options.tile_waves / tile_mode
// pin it).  Few tiles cannot fill the GPU with four waves each: more waves per tile shorten every
// wave's serial chain, and sharing the bin between them (instead of giving each a column of the
// tile) keeps them equally loaded where polygons cluster.  Many tiles fill the GPU anyway: four
// waves with private columns do the least total work.  Measured on diablo / phong (k_tile us, best
// of the six combinations per size, profiles/r02_notes.md): 512^2 24.8 (16 shared; 4 columns 129),
// 1024^2 22.2 (16 shared), 2048^2 21.9 (8 shared), 2560^2 23.2 (8 columns), 4096^2 33.1 (4 columns).
// A fused launch (tr_scene_render_frames) fills the GPU with the tiles of ALL its frames, so its waves per
// tile go by that total; whether its waves share a tile's bin still goes by the size of ONE frame, which is
// what decides how unevenly the polygons fall on a tile's columns (800^2 african_head, 16 frames per launch,
// k_tile per frame: 4 waves columns 4.6 us, 4 waves shared 3.3, 8 shared 3.6, 16 shared 4.4) ...
void tile_layout(const tr_scene *s, uint64_t tiles_in_launch, uint32_t tiles_per_frame, uint32_t n_poly, int &tile_waves, int &shared)
{
    tile_waves = s->tile_waves ? (int)s->tile_waves : tiles_in_launch <= 1024u ? 16 : tiles_in_launch <= 4608u ? 8 : 4;
    // ... or by how many polygons a tile gets: many small ones are visited once per tile instead of once per
    // column they touch.  k_tile per frame, columns -> shared, polygons per tile of the frame: 8192^2 x64 grid
    // specular (9.8) 371 -> 350 us, the same with phong 259 -> 230, 4096^2 x16 (9.8) 66.9 -> 60.0, x9 (5.5)
    // 50.4 -> 47.6, x4 (2.5) 38.9 -> 38.5, one model (0.6) 33.5 -> 35.4
    const bool dense = (uint64_t)n_poly >= 3ull * (tiles_per_frame ? tiles_per_frame : 1u);
    shared = s->tile_mode ? (s->tile_mode == 2 ? 1 : 0) : tile_mode_auto((tiles_per_frame <= 2048u || dense) ? 1 : 0);
    // the shared keys pack polygon id and bin slot into 32 bits: beyond their fields, resolve by columns.  Decided
    // HERE, once per pass: k_setup prepares the pairs' masks for the form the tile kernel will run (SetupArgs::cells)
    if (n_poly > (1u << 20)) shared = 0;  // (a TILE with more records than the slot field holds resolves by columns: k_tile)
}

// May a cleared frame's colour pass leave its depth on the chip?  Not with the winner tap or the tile stamps (single
// diagnostic buffers whose tests read the z buffer after every frame: nothing to gain).
bool defer_depth(const tr_scene *s)
{
    static const int env_on = getenv("TR_DEFER_Z") ? atoi(getenv("TR_DEFER_Z")) : 1;
    return env_on && s->transient_depth && !s->d_winner && !s->d_stamps;
}

// (TR_FUSED_SINGLE=0: a per-frame pass runs the per-frame kernels whatever its targets' state, as before round 4)
static bool fused_single_launches()
{
    static const bool on = !getenv("TR_FUSED_SINGLE") || atoi(getenv("TR_FUSED_SINGLE")) != 0;
    return on;
}

// A slot's shadow buffer is about to be rendered under shadow matrix `m` (16 floats).
void note_shadow_matrix(tr_scene::FrameSlot &slot, const float *m)
{
    memcpy(slot.shadow_matrix, m, sizeof slot.shadow_matrix);
    slot.shadow_matrix_set = true;
}

// One frame's render targets, as fill_pass_args takes them: run_pass passes the scene's current aliases (s->d_*),
// run_group a frame slot's buffers with the colour target and flags it has resolved for the frame.
struct PassTargets {
    float *z, *shadow;
    uint8_t *fb;
    uint32_t *zclean, *sclean, *fbclean;
    uint32_t *winner;
    uint64_t *stamps;
};

// The storage of one pass's chain: run_pass passes its share of the LOOKAHEAD rings and the BinState's counter set,
// run_group slice e of the GroupSet.  lit: where the frame's lit image goes (scenes on the lit path).  len_src / len_host:
// SetupArgs' -- a fused launch reports its list lengths to the host; null on the per-frame path.
struct ChainStore {
    uint32_t *tile_count;
    Piece *recs, *bins;
    WorkItem *order;
    uint32_t *lit;
    const uint32_t *len_src;
    uint32_t *len_host;
};

// The arguments of one pass of one frame: every member of `sa` but sa.u, which the caller has filled in place
// (pass_uniforms: the constants are copied once, into ta.u), and every member of `ta`.  Decides nothing: whether the
// targets are cleared (fresh), what the pass writes (store), the tile kernel's form (shared) and which targets and
// storage are the callers'.  depth_only (ensure_depth's repeat): no winner words, no stamps, and the pass's own closure
// -- no lit arguments -- even on a scene whose lit path is on.  Allocates nothing.
void fill_pass_args(const tr_scene *s, const PassDesc &p, const PassTargets &t, const ChainStore &c, const DevMesh &mesh, int shared,
                    uint32_t fresh, uint32_t store, uint64_t pass_seq, bool depth_only, SetupArgs &sa, TileArgs &ta)
{
    const bool depth_pass = p.fs == FS_DEPTH;
    const bool looks_up_shadow = p.fs == FS_SHADOW2 || p.fs == FS_OCCLUSION2;
    const bool lit = !depth_only && tile_fs(s, p.fs) == (int)FS_LIT;   // k_lit runs the closure per texel, the tiles fetch its result
    const DevFrame &frame = depth_pass ? s->frame_full : s->frame;      // (a depth pass fills the whole shadow buffer)
    sa.mesh = mesh;
    sa.frame = frame;
    sa.tile_count = c.tile_count;
    sa.recs = c.recs;
    sa.bins = c.bins;
    sa.pool_cap = s->pool_cap;
    sa.rec_pieces = s->rec_pieces;
    sa.err = s->d_err;
    sa.alarm = s->d_alarm;
    sa.cells = shared ? 1u : 0u;
    sa.lit = lit ? c.lit : nullptr;
    sa.texel_set = lit ? s->tex.packed : nullptr;
    sa.tex_w = lit ? s->tex.w[0] : 0u;
    sa.tex_h = lit ? s->tex.h[0] : 0u;
    sa.set_bpr = lit ? s->set_bpr : 0u;
    sa.lit_bpr = lit ? s->lit_bpr : 0u;
    sa.len_src = c.len_src;
    sa.len_host = c.len_host;
    memset(&ta, 0, sizeof ta);   // (list_len: zeroed by the host, filled by k_order)
    ta.bins = c.bins;
    ta.pool_cap = s->pool_cap;
    ta.rec_pieces = s->rec_pieces;
    ta.order = c.order;
    ta.tile_count = c.tile_count;
    ta.bin_need = s->d_bin_need;
    ta.overflow_seq = s->d_overflow_seq;
    ta.pass_seq = pass_seq;
    ta.frame = frame;
    ta.u = sa.u;
    ta.tex = s->tex;
    if (lit) {
        ta.tex.packed = c.lit;   // (one word per texel, 8x4 blocks: what fetch_texels<FS_LIT> reads)
        ta.tex.packed_bpr = s->lit_bpr;
    }
    ta.zbuf = t.z;
    ta.shadow = t.shadow;
    ta.fb = t.fb;
    ta.winner = depth_only ? nullptr : t.winner;
    ta.err = s->d_err;
    ta.alarm = s->d_alarm;
    ta.fresh = fresh;
    ta.store = store;
    ta.aligned16 = (s->width % 16u == 0u) ? 1u : 0u;
    ta.aligned4 = (s->width % 4u == 0u) ? 1u : 0u;
    ta.stamps = (depth_pass || depth_only) ? nullptr : t.stamps;
    ta.zclean = depth_pass ? t.sclean : t.zclean;   // (the depth pass's z is the shadow buffer)
    ta.fbclean = depth_pass ? nullptr : t.fbclean;
    ta.sclean = looks_up_shadow ? t.sclean : nullptr;
}

// Queues one pass's chain on `chain`: k_lit first where the pass is lit (sa0.lit: it needs nothing but the frame's
// constants), then vertex stage + counting, work lists + pool ranges, records into the ranges.  d_setup / d_tile: the
// device tables of a fused launch over g frames -- sa0 / ta0 then say what the frames share, n_poly is the largest
// frame's and xform whether any frame draws a transform table -- or null: the one frame sa0 / ta0 describe (g = 1).
// `done` (may be null) completes with the chain.  Without profiling it rides on the last kernel's own completion signal
// -- k_bin's, or k_order's when there are no polygons and k_bin is not launched; with profiling the kernels carry their
// timing events and `done` is recorded behind them.
int launch_chain(tr_scene *s, const PassDesc &p, const SetupArgs &sa0, const TileArgs &ta0, const SetupArgs *d_setup, const TileArgs *d_tile,
                 uint32_t g, uint32_t n_tiles_pass, uint32_t n_poly, bool xform, bool chain_on_main, hipStream_t chain, hipEvent_t done)
{
    const uint32_t nf = d_setup ? g : 0u;   // (the launchers' n_frames: 0 = an ordinary launch)
    const bool prof = s->profiling;
    if (sa0.lit) {
        const EventPair el = timing_pair(s, K_LIT, g);
        int rc = launch_lit(p.fs, sa0, d_setup, nf, chain, el.a, el.b);
        if (rc) return launch_status(rc, "k_lit");
        if (prof) s->events.push_back(el);
    }
    const EventPair ep = timing_pair(s, K_SETUP, g);
    int rc = launch_setup(p.vs, sa0, d_setup, nf, xform, chain_on_main, chain, ep.a, ep.b);
    if (rc) return launch_status(rc, "k_setup");
    if (prof) s->events.push_back(ep);
    const EventPair eo = timing_pair(s, K_ORDER, g);
    rc = launch_order(ta0, n_tiles_pass, d_tile, nf, chain, eo.a, (prof || n_poly) ? eo.b : done);
    if (rc) return launch_status(rc, "k_order");
    if (prof) s->events.push_back(eo);
    if (n_poly) {
        const EventPair eb = timing_pair(s, K_BIN, g);
        rc = launch_bin(sa0, d_setup, nf, chain_on_main, chain, eb.a, prof ? eb.b : done);
        if (rc) return launch_status(rc, "k_bin");
        if (prof) s->events.push_back(eb);
    }
    if (prof && done) HIP_TRY(hipEventRecord(done, chain));
    return TR_OK;
}

// depth_only: the repeat of a colour pass for its depth alone (ensure_depth): from cleared targets, nothing of the
// scene's clear / colour state is consumed or changed.
int run_pass(tr_scene *s, const PassDesc &p, bool depth_only = false)
{
    SetupArgs sa = {};   // (every byte defined: the kernels take the struct by value)
    int st = pass_uniforms(s, p, sa.u);
    if (st != TR_OK) return st;
    // a per-frame pass after frame groups: their tile kernels first (it may render onto their targets)
    if (s->group_submitted < s->group_seq || s->groups_unfenced) {
        st = finish_groups(s);
        if (st != TR_OK) return st;
    }

    const bool depth_pass = (p.fs == FS_DEPTH);
    // Which targets does this pass write, and are they logically cleared?
    uint32_t fresh;
    if (depth_pass) {
        fresh = s->shadow_cleared ? 1u : 0u;
        s->shadow_cleared = false;
        note_shadow_matrix(s->slots[(size_t)s->cur_slot], sa.u.shadow_matrix);
    } else if (depth_only) {
        fresh = 1u;
    } else {
        fresh = s->z_fb_cleared ? 1u : 0u;
        s->z_fb_cleared = false;
        // a colour pass that reads the shadow buffer needs real values in it
        if (p.fs == FS_SHADOW2 || p.fs == FS_OCCLUSION2) {
            st = flush_clear_shadow(s);
            if (st != TR_OK) return st;
        }
    }

    const DevFrame &frame = depth_pass ? s->frame_full : s->frame;

    const uint32_t n_tiles_pass = frame.ntx * frame.nty;
    tr_scene::PendingTile pt;
    tile_layout(s, n_tiles_pass, n_tiles_pass, s->mesh.n_tri, pt.tile_waves, pt.shared);
    pt.n_poly = s->mesh.n_tri;

    // What the pass writes to memory (TileArgs::store)
    uint32_t store = TR_STORE_DEPTH | TR_STORE_COLOR;
    if (!depth_pass) {
        tr_scene::FrameSlot &slot = s->slots[(size_t)s->cur_slot];
        if (depth_only) {
            store = TR_STORE_DEPTH;
            slot.z_deferred = false;
        } else if (fresh && !s->d_winner && defer_depth(s) && fused_single_launches()) {
            // a cleared frame on its own: the fused launches' kernel for one frame (launch_tile, fused_single), and like
            // a group's frames it leaves its depth on the chip; whoever wants the z buffer gets it from ensure_depth
            store = TR_STORE_COLOR;
            slot.z_deferred = true;
            slot.z_params = s->view;
            slot.z_inst = s->inst;
        } else {
            // (an accumulating render has had the slot's depth made real before it came here: ensure_depth, tr_scene_render)
            slot.z_deferred = false;
        }
    }
    pt.fused_single = !depth_only && fresh != 0u && !s->d_winner && fused_single_launches();
    if (!depth_pass && ((store & TR_STORE_DEPTH) || fresh == 0u)) {   // the pass reads or writes z memory
        st = need_z(s, s->cur_slot);
        if (st != TR_OK) return st;
    }
    tr_scene::BinState &bs = depth_pass ? s->bin_depth : s->bin_color;
    const uint64_t p_seq = s->pass_seq;
    const size_t ring = (size_t)(p_seq % LOOKAHEAD);
    // (the current aliases, read after need_z: it may have given the slot its z buffer and pointed d_z at it)
    const PassTargets targets = { s->d_z, s->d_shadow, s->d_fb, s->d_zclean, s->d_sclean, s->d_fbclean, s->d_winner, s->d_stamps };
    const ChainStore cs = { bs.count[bs.seq % SETS], s->d_recs[ring], s->d_bins[ring], s->d_order[ring], s->d_lit[ring], nullptr, nullptr };
    TileArgs &ta = pt.args;
    fill_pass_args(s, p, targets, cs, s->mesh, pt.shared, fresh, store, p_seq, depth_only, sa, ta);
    // setup on its own stream: after the tile kernel of pass p - LOOKAHEAD, before the tile kernel of pass p.
    // With NOTHING in flight (a frame rendered and read, rendered and read: the interactive loop) the chain has
    // nothing to overlap with, and the hop between the streams -- event, wait packet, dispatch: 13-17 us -- is
    // pure latency: then setup, work list and tiles go down the main stream in order.
    // "Nothing in flight" is what the host KNOWS after it has waited for the stream (a loop that merely runs
    // ahead of a fast GPU must keep its overlap: asking the stream instead cost small frames 7-16 %).
    const bool chain_on_main = s->own_stream && s->quiescent && s->pending.empty() && s->group_submitted == s->group_seq;
    s->quiescent = false;
    hipStream_t chain = chain_on_main ? s->stream : (s->two_setup_streams && (p_seq & 1u)) ? s->setup_stream2 : s->setup_stream;
    if (!chain_on_main && p_seq >= (uint64_t)LOOKAHEAD)
        HIP_TRY(hipStreamWaitEvent(chain, s->ev_tile[(p_seq - LOOKAHEAD) % RING], 0));
    // the pose's rows first (once per pose: the passes of a frame read the same rows)
    if (s->inst.pose) {
        if ((st = blend_poses(s, &s->inst.pose, 1u, chain)) != TR_OK) return st;
        sa.mesh.tri = s->mesh.tri = s->inst.pose->rows.d;
    }
    if (!sa.mesh.tri && sa.mesh.n_tri) return tr::fail(TR_E_INVALID, "no rows to draw");
    st = launch_chain(s, p, sa, ta, nullptr, nullptr, 1u, n_tiles_pass, sa.mesh.n_tri, sa.mesh.inst_xform != 0u, chain_on_main, chain,
                      s->ev_setup[p_seq % RING]);
    if (st != TR_OK) return st;
    if ((st = note_inst_use(s, sa.mesh, chain)) != TR_OK) return st;
    if ((st = note_pose_use(s, &s->inst.pose, 1u, chain)) != TR_OK) return st;
    pt.fs = depth_only ? p.fs : tile_fs(s, p.fs);
    pt.kernel_id = depth_pass ? K_TILE_DEPTH : K_TILE;
    pt.p_seq = p_seq;
    s->pending.push_back(pt);
    bs.seq++;
    s->pass_seq++;
    // a caller's stream must hold the frame when render() returns (its next operation may consume
    // it: from here on the pass counts as handed on, see recover_from_overflow)
    if (!s->own_stream) {
        s->observed_seq = s->pass_seq;
        return submit_pending_tiles(s);
    }
    // the library's own stream: see "Handing tile kernels to the main stream" above
    if (chain_on_main) return submit_front(s, false);  // its setup is ahead of it in the same queue
    // (tr_plan.h, handover: the three cases of "Handing tile kernels to the main stream" above)
    switch (plan::handover(s->pending.size(), s->tiles_submitted == 0,
                           s->tiles_submitted != 0 && hipEventQuery(s->ev_tile[s->last_submitted_seq % RING]) == hipSuccess)) {
    case plan::Handover::HOST_WAITS: {
        // steady state: the HOST waits for the oldest pending pass's setup (it completed long ago, or will
        // within microseconds: the setup stream runs ahead, and the main stream still holds the tile kernels
        // of the passes before it), then its tile kernel goes out with no wait packet in the GPU's queue.
        // This is also what keeps the host from running ahead of the GPU without bound.
        int status = TR_OK;
        while ((int)s->pending.size() > BATCH) {
            HIP_TRY(hipEventSynchronize(s->ev_setup[s->pending.front().p_seq % RING]));
            int st2 = submit_front(s, false);
            if (st2 != TR_OK && status == TR_OK) status = st2;
        }
        return status;
    }
    case plan::Handover::FRONT_WITH_WAIT:
        // start-up (the first passes after a sync): a main stream that has run dry gets the next tile kernel
        // behind a wait packet (an idle GPU loses nothing to it) ...
        return submit_front(s, true);
    case plan::Handover::READY_ONLY:
        break;
    }
    // ... otherwise whatever has its setup behind it goes out without one
    return submit_ready(s);
}

int render_frame(tr_scene *s)
{
    s->host_status = TR_OK;
    const PipelineDesc &pd = kPipelines[s->pipeline];
    for (int i = 0; i < pd.n_passes; i++) {
        int st = run_pass(s, pd.pass[i]);
        if (st != TR_OK) {
            s->host_status = st;
            return st;
        }
    }
    return TR_OK;
}

// Makes the current slot's z buffer real.  A cleared frame's colour pass leaves its depth on the chip (transient depth:
// nothing reads the z buffer of such a frame -- the next cleared frame overwrites it unseen); the first consumer that
// does want it -- tr_scene_read_z_f32 / tr_scene_get_z_buffer, a render WITHOUT a clear, which depth-tests against it
// (scene.rs:151) -- repeats the frame's colour pass for the depth alone: same light and camera, same cull and
// projection, same resolve; colour, winner words, flags of the frame buffer and the scene's clear state untouched.
int ensure_depth(tr_scene *s)
{
    tr_scene::FrameSlot &slot = s->slots[(size_t)s->cur_slot];
    if (!slot.z_deferred) return TR_OK;
    int st = submit_pending(s);   // (the frame itself, should it still be held back)
    if (st != TR_OK) return st;
    if (!slot.z_deferred) return TR_OK;
    const DrawState now(s);
    s->view = slot.z_params;
    use_inst(s, slot.z_inst);
    const PipelineDesc &pd = kPipelines[s->pipeline];
    const int host_status = s->host_status;
    st = run_pass(s, pd.pass[pd.n_passes - 1], true);
    if (st == TR_OK) st = submit_pending_tiles(s);
    s->host_status = host_status;
    return st;
}


// ---------------------------------------------------------------------------------------------
// Frame groups (tr_scene_render_frames)
// ---------------------------------------------------------------------------------------------

// Frames per fused launch: enough tiles to keep the machine full while one frame's light tiles drain and to
// make the gap between launches small against the launch -- 32 K tiles (4096^2: 4 frames, 8 no better; 3072^2
// 4 -> 8 frames 19.0 -> 18.1 us per frame, 2048^2 8 -> 16 10.4 -> 10.0, 1536^2 14 -> 28 7.2 -> 6.8), within
// GROUP_MAX; at least four frames.  The winner tap and the tile stamps are single buffers: one frame.
plan::SceneShape shape_of(const tr_scene *s)
{
    static const int forced = getenv("TR_GROUP") ? atoi(getenv("TR_GROUP")) : 0;  // experiment hook
    plan::SceneShape q;
    q.n_tiles = s->n_tiles;
    q.frames_per_launch = s->frames_per_launch;
    q.max_slots = s->max_slots;
    q.forced = forced > 0 ? (uint32_t)forced : 0u;
    q.winner_tap = s->d_winner != nullptr;
    q.tile_stamps = s->d_stamps != nullptr;
    q.no_long_runs = s->no_long_runs;
    q.n_passes = (uint32_t)kPipelines[s->pipeline].n_passes;
    q.pool_bytes_per_pass = (uint64_t)s->pool_cap * s->rec_pieces * 16ull;
    q.pixels = (uint64_t)s->width * s->height;
    return q;
}

uint32_t group_size(const tr_scene *s) { return plan::group_size(shape_of(s)); }

// Frames per launch that a LONG run of frames grows to (tr_scene_render_frames with sixteen groups or more; the
// per-frame protocol after sixteen full groups in a row): between two tile kernels of a stream lie 6-12 us (the end of
// a kernel that wrote 200 MB, the dispatch of the next), paid once per launch -- 32 frames per launch instead of 4 make
// 4096^2 30.1 -> 28.7 us per frame.  Only when the group size is automatic, within 8 GiB of frame slots and 16 GiB of
// record pools.  (Not for short runs: a slot's first frames are slower than its later ones -- 20 frames into 20 slots:
// tile kernel 31.2 us per frame, into 4 slots used five times each: 29.1.)
uint32_t long_run_group_size(const tr_scene *s) { return plan::long_run_group_size(shape_of(s)); }

// Frame slots 1 .. n - 1 (slot 0 exists since tr_scene_create).  Their z memory needs no initial value:
// a slot is only ever reached through a group's cleared frame, which writes every tile or raises its flag.
int ensure_slots(tr_scene *s, uint32_t n)
{
    const size_t npx = (size_t)s->width * s->height;
    while (s->slots.size() < n) {
        tr_scene::FrameSlot fs;
        // (no z buffer yet: need_z)
        int st = dev_alloc(&fs.zclean, (size_t)s->n_tiles);
        if (st == TR_OK && kPipelines[s->pipeline].n_passes == 2) st = dev_alloc(&fs.shadow, npx);
        if (st == TR_OK && kPipelines[s->pipeline].n_passes == 2) st = dev_alloc(&fs.sclean, (size_t)s->n_tiles_full);
        if (st != TR_OK) {
            dev_free(fs.z);
            dev_free(fs.zclean);
            dev_free(fs.shadow);
            dev_free(fs.sclean);
            return st;
        }
        if (!fs.shadow) {  // never written without a depth pass
            fs.shadow = s->slots[0].shadow;
            fs.sclean = s->slots[0].sclean;
        }
        s->slots.push_back(fs);
    }
    return TR_OK;
}

size_t group_bins_per_frame(const tr_scene *s) { return (size_t)s->pool_cap * s->rec_pieces; }
size_t group_recs_per_frame(const tr_scene *s) { return (size_t)(s->poly_cap ? s->poly_cap : 1u) * s->rec_pieces; }
size_t group_counts_per_frame(const tr_scene *s) { return (size_t)s->n_tiles_full + 16u; }

void free_group_set(tr_scene::GroupSet &gs);

int ensure_group_set(tr_scene *s, tr_scene::GroupSet &gs, uint32_t frames)
{
    const size_t np = (size_t)kPipelines[s->pipeline].n_passes;
    if (!gs.ev_setup) {
        HIP_TRY(hipEventCreateWithFlags(&gs.ev_setup, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&gs.ev_tile, hipEventDisableTiming));
    }
    int st = TR_OK;
    if ((gs.frames < frames || gs.pool_cap != s->pool_cap) && gs.in_flight) {
        HIP_TRY(hipEventSynchronize(gs.ev_tile));  // its memory is about to be replaced
        gs.in_flight = false;
    }
    if (gs.frames < frames) {
        free_group_set(gs);
        const size_t nc = np * frames * group_counts_per_frame(s);
        if ((st = dev_alloc(&gs.count, nc))) return st;
        // (from here on every tile kernel workgroup zeroes its tile's counter.)  hipMemset returns before the device has
        // executed it and the scene's streams do not wait for the null stream: without the synchronisation the
        // set's first k_setup could count on top of whatever the fresh allocation held (an intermittent "bin
        // overflow" the first time a fourth group was in flight)
        HIP_TRY(hipMemset(gs.count, 0, nc * 4));
        HIP_TRY(hipStreamSynchronize(nullptr));
        if ((st = dev_alloc(&gs.order, np * frames * (size_t)s->n_tiles_full * ORDER_LISTS))) return st;
        if ((st = dev_alloc(&gs.recs, np * frames * group_recs_per_frame(s)))) return st;
        dev_free(gs.lit);
        if (s->lit && (st = dev_alloc(&gs.lit, np * frames * (size_t)s->lit_words))) return st;
        const size_t tb = np * frames * (sizeof(SetupArgs) + sizeof(TileArgs));
        if ((st = dev_alloc(&gs.d_tables, tb))) return st;
        HIP_TRY(hipHostMalloc((void **)&gs.h_tables, tb, hipHostMallocDefault));
        {
            void *h = nullptr, *d = nullptr;
            HIP_TRY(hipHostMalloc(&h, np * frames * LEN_WORDS * sizeof(uint32_t), hipHostMallocMapped));
            memset(h, 0, np * frames * LEN_WORDS * sizeof(uint32_t));
            HIP_TRY(hipHostGetDevicePointer(&d, h, 0));
            gs.h_lens = (volatile uint32_t *)h;
            gs.d_lens = (uint32_t *)d;
        }
        gs.frames = frames;
    }
    if (gs.pool_cap != s->pool_cap) {
        dev_free(gs.bins);
        gs.pool_cap = 0;
        if ((st = dev_alloc(&gs.bins, np * gs.frames * group_bins_per_frame(s)))) return st;
        gs.pool_cap = s->pool_cap;
    }
    return TR_OK;
}

int slot_own_fb(tr_scene *s, int k, uint8_t **out);

// Everything a long run's large groups need -- frame slots with their colour buffers, the sets of the groups in
// flight -- allocated once, the first time the scene sees frames in bulk (a tr_scene_render_frames call of more than
// one group, or a group that filled up under the per-frame protocol): a few milliseconds and, at 4096^2, 4 GiB that a
// later, longer run must not pay for in its own time (a warm-up of five frames, then the timed twenty or two thousand).
void free_group_set(tr_scene::GroupSet &gs)
{
    dev_free(gs.count);
    dev_free(gs.order);
    dev_free(gs.recs);
    dev_free(gs.lit);
    dev_free(gs.d_tables);
    if (gs.h_tables) (void)hipHostFree(gs.h_tables);
    gs.h_tables = nullptr;
    if (gs.h_lens) (void)hipHostFree((void *)gs.h_lens);
    gs.h_lens = nullptr;
    gs.d_lens = nullptr;
    dev_free(gs.bins);
    gs.pool_cap = 0;
    gs.frames = 0;
}

int prepare_long_runs(tr_scene *s, bool own_colour)
{
    const uint32_t g = long_run_group_size(s);
    if (g <= group_size(s) || s->d_winner) return TR_OK;
    const size_t slots_before = s->slots.size();
    int st = ensure_slots(s, g);
    for (uint32_t k = 0; k < g && st == TR_OK && own_colour; k++) {
        uint8_t *unused = nullptr;
        st = slot_own_fb(s, (int)k, &unused);
    }
    for (int k = 0; k < GROUP_SETS && st == TR_OK; k++) st = ensure_group_set(s, s->grp[k], g);
    if (st != TR_E_NOMEM) return st;
    // The device has no room for a long run's resources (a smaller GPU, several scenes or ranks on one): give back
    // what was taken just now -- nothing has used it -- and go on with the usual groups, for good.
    const std::string why = tr::g_last_error;
    (void)hipStreamSynchronize(s->stream);  // (the new colour buffers' zero fill)
    const uint32_t G = group_size(s);
    while (s->slots.size() > slots_before && s->slots.size() > (size_t)G) {
        tr_scene::FrameSlot &fs = s->slots.back();
        if (fs.fb)
            for (size_t k = 0; k < s->fb_flags.size(); k++)
                if (s->fb_flags[k].fb == fs.fb && s->fb_flags[k].clean != s->d_fbclean) {
                    dev_free(s->fb_flags[k].clean);
                    s->fb_flags.erase(s->fb_flags.begin() + (long)k);
                    break;
                }
        dev_free(fs.z);
        dev_free(fs.zclean);
        if (fs.shadow != s->slots[0].shadow) {
            dev_free(fs.shadow);
            dev_free(fs.sclean);
        }
        dev_free(fs.fb);
        s->slots.pop_back();
    }
    for (tr_scene::GroupSet &gs : s->grp)
        if (!gs.in_flight && gs.frames > G) free_group_set(gs);
    s->no_long_runs = true;
    tr::g_last_error = "large frame groups disabled for this scene: " + why;
    return TR_OK;
}

int submit_groups(tr_scene *s, bool all);

// (TR_WORK_UNITS=0: every tile kernel is launched with one workgroup per tile, as before round 4)
static bool use_work_units()
{
    static const bool on = !getenv("TR_WORK_UNITS") || atoi(getenv("TR_WORK_UNITS")) != 0;
    return on;
}

// Workgroups per frame for the tile kernels of pass `pi` of the group in `gs`, whose chain HAS COMPLETED (the caller has
// seen its event), or 0: one per tile.  The tile kernel needs one workgroup per WORK UNIT -- a tile with polygons, or
// EMPTY_CHUNK empty tiles (tr_kernels.hip) -- and k_bin_group, the chain's last kernel, has left every frame's list
// lengths in page-locked memory: the frame that needs most decides (a fused launch's frames share the grid).
static uint32_t group_units(const tr_scene *s, const tr_scene::GroupSet &gs, uint32_t pi, uint32_t n_tiles_pass)
{
    if (!gs.h_lens || gs.n_poly == 0 || gs.g > (uint32_t)GROUP_MAX) return 0u;  // (no polygons: no k_bin)
    uint32_t lens[GROUP_MAX * LEN_WORDS];
    const volatile uint32_t *w = gs.h_lens + (size_t)pi * gs.frames * LEN_WORDS;
    for (uint32_t i = 0; i < gs.g * LEN_WORDS; i++) lens[i] = w[i];
    return plan::group_grid_units(lens, gs.g, n_tiles_pass);
}

// Queues the setup of g <= frames-per-group cleared frames, one launch per kernel and pass.  Frame j takes
// light and camera from p[j], its instance table from insts[j] (insts == null: the scene's current one), its targets
// from slot slot_of[j] and its colour buffer from fbs[j] (fbs == null: the slot's own).  The tile kernels follow with
// submit_groups.
int run_group(tr_scene *s, const tr_frame_params *p, const tr_scene::InstRef *insts, void *const *fbs, const int *slot_of, uint32_t g,
              bool forget_callers_buffers = false)
{
    const PipelineDesc &pd = kPipelines[s->pipeline];
    const uint32_t np = (uint32_t)pd.n_passes;
    tr_scene::GroupSet &gs = s->grp[s->group_seq % GROUP_SETS];
    // nothing in flight (the first group after a sync): its setup goes down the main stream, ahead of its tile
    // kernels, without the hop between the streams (see run_pass)
    const bool chain_on_main = s->own_stream && s->quiescent && s->pending.empty() && s->group_submitted == s->group_seq;
    s->quiescent = false;
    // the set's previous group must have left the GPU before its bins, counters and tables are written again;
    // this wait is also what keeps the host from running ahead of the GPU without bound
    if (gs.in_flight) {
        // (about to wait on the host: whatever tile kernels are still held back go to the device first -- a wait
        // packet in front of them costs less than a GPU that runs dry while the host sleeps)
        if (s->group_seq - s->group_submitted >= (uint64_t)GROUP_SETS || hipEventQuery(gs.ev_tile) != hipSuccess) {
            int sg = submit_groups(s, true);
            if (sg != TR_OK) return sg;
        }
        HIP_TRY(hipEventSynchronize(gs.ev_tile));
    }
    gs.in_flight = false;
    int st = ensure_group_set(s, gs, g > group_size(s) ? g : group_size(s));
    if (st != TR_OK) return st;
    const uint32_t G = gs.frames;
    if (g == 0 || g > G) return tr::fail(TR_E_INVALID, "group larger than its set");

    SetupArgs *h_setup = reinterpret_cast<SetupArgs *>(gs.h_tables);
    TileArgs *h_tile = reinterpret_cast<TileArgs *>(gs.h_tables + (size_t)np * G * sizeof(SetupArgs));
    const SetupArgs *d_setup = reinterpret_cast<const SetupArgs *>(gs.d_tables);
    const TileArgs *d_tile = reinterpret_cast<const TileArgs *>(gs.d_tables + (size_t)np * G * sizeof(SetupArgs));

    // the frames share the launches' grids: the one with most polygons sizes them
    uint32_t n_poly = 0;
    for (uint32_t j = 0; j < g; j++) {
        const uint32_t n = mesh_of(s, insts ? insts[j] : s->inst).n_tri;
        n_poly = n > n_poly ? n : n_poly;
    }
    for (uint32_t pi = 0; pi < np; pi++) {
        const DevFrame &fr = pd.pass[pi].fs == FS_DEPTH ? s->frame_full : s->frame;
        tile_layout(s, (uint64_t)fr.ntx * fr.nty * g, fr.ntx * fr.nty, n_poly, gs.tile_waves[pi], gs.shared[pi]);
    }
    const DrawState now(s);  // (every frame's view passes through s->view, which pass_uniforms reads; nothing below the loop does)
    for (uint32_t j = 0; j < g && st == TR_OK; j++) {
        s->view = p[j];
        if (!defer_depth(s)) st = need_z(s, slot_of[j]);   // (the frames store their depth)
        if (st != TR_OK) break;
        tr_scene::FrameSlot &slot = s->slots[(size_t)slot_of[j]];
        slot.z_deferred = defer_depth(s);   // (what the slot's z is then: this frame)
        slot.z_params = p[j];
        slot.z_inst = insts ? insts[j] : s->inst;
        if (slot.z_inst.pose && (st = pose_rows(s, *slot.z_inst.pose)) != TR_OK) break;
        const DevMesh mesh = mesh_of(s, slot.z_inst);
        if (!mesh.tri && mesh.n_tri) {
            st = tr::fail(TR_E_INVALID, "no rows to draw");
            break;
        }
        uint8_t *fb = fbs ? (uint8_t *)fbs[j] : nullptr;
        const bool callers = fb != nullptr;
        if (!fb) st = slot_own_fb(s, slot_of[j], &fb);
        uint32_t *fbclean = nullptr;
        if (st == TR_OK) st = fb_flags_for(s, fb, &fbclean, callers && forget_callers_buffers);
        // (the slot's z after need_z.  The winner tap is null on every way here: with it render_frames and replay_tail go
        // frame by frame through run_pass, and frame_is_groupable holds no frame back)
        const PassTargets targets = { slot.z, slot.shadow, fb, slot.zclean, slot.sclean, fbclean, s->d_winner, s->d_stamps };
        for (uint32_t pi = 0; pi < np && st == TR_OK; pi++) {
            const PassDesc &pass = pd.pass[pi];
            const size_t e = (size_t)pi * G + j;  // this frame-pass's share of the set
            SetupArgs &sa = h_setup[e];
            st = pass_uniforms(s, pass, sa.u);
            if (st != TR_OK) break;
            if (pass.fs == FS_DEPTH) note_shadow_matrix(slot, sa.u.shadow_matrix);
            const ChainStore cs = { gs.count + e * group_counts_per_frame(s), gs.recs + e * group_recs_per_frame(s),
                                    gs.bins + e * group_bins_per_frame(s), gs.order + e * (size_t)s->n_tiles_full * ORDER_LISTS,
                                    gs.lit ? gs.lit + e * (size_t)s->lit_words : nullptr, d_tile[e].list_len, gs.d_lens + e * LEN_WORDS };
            // every frame of a group starts from cleared targets; its colour pass leaves the depth on the chip where it may;
            // passes are numbered frame by frame, as the per-frame path numbers them
            const uint32_t store = (pass.fs != FS_DEPTH && defer_depth(s)) ? TR_STORE_COLOR : (TR_STORE_DEPTH | TR_STORE_COLOR);
            fill_pass_args(s, pass, targets, cs, mesh, gs.shared[pi], 1u, store, s->pass_seq + (uint64_t)j * np + pi, false, sa, h_tile[e]);
        }
    }
    if (st != TR_OK) return st;

    // tables to the device, then per pass: vertex stage + binning of all frames, their work lists
    hipStream_t chain = chain_on_main ? s->stream : s->setup_stream;
    // the frames' poses: blended by one launch ahead of the chain that reads their rows (both passes of a frame do)
    std::shared_ptr<tr_scene::Pose> poses[GROUP_MAX];
    for (uint32_t j = 0; j < g; j++) poses[j] = s->slots[(size_t)slot_of[j]].z_inst.pose;
    if ((st = blend_poses(s, poses, g, chain)) != TR_OK) return st;
    HIP_TRY(hipMemcpyAsync(gs.d_tables, gs.h_tables, (size_t)np * G * (sizeof(SetupArgs) + sizeof(TileArgs)),
                           hipMemcpyHostToDevice, chain));
    for (uint32_t pi = 0; pi < np; pi++) {
        const PassDesc &pass = pd.pass[pi];
        // (the launches' shape: the first frame's arguments with the group's largest polygon count; every frame's
        // kernels read their own entry of the table)
        SetupArgs sa0 = h_setup[(size_t)pi * G];
        sa0.mesh.n_tri = n_poly;
        bool xform = false;  // does any frame of the group draw a transform table?
        for (uint32_t j = 0; j < g; j++) xform = xform || h_setup[(size_t)pi * G + j].mesh.inst_xform != 0u;
        // (no `done`: one record behind all the passes' chains, below)
        st = launch_chain(s, pass, sa0, h_tile[(size_t)pi * G], d_setup + (size_t)pi * G, d_tile + (size_t)pi * G, g,
                          sa0.frame.ntx * sa0.frame.nty, n_poly, xform, chain_on_main, chain, nullptr);
        if (st != TR_OK) return st;
    }
    HIP_TRY(hipEventRecord(gs.ev_setup, chain));
    for (uint32_t j = 0; j < g; j++)
        if ((st = note_inst_use(s, h_setup[j].mesh, chain)) != TR_OK) return st;
    if ((st = note_pose_use(s, poses, g, chain)) != TR_OK) return st;
    gs.chain_on_main = chain_on_main;
    gs.g = g;
    gs.n_poly = n_poly;
    gs.in_flight = true;
    s->pass_seq += (uint64_t)g * np;
    s->group_seq++;
    return TR_OK;
}

// The tile kernels of the oldest group whose setup is queued, pass by pass (a colour pass reads what its
// frame's depth pass wrote), behind a wait for that setup unless the caller knows it has completed.
int submit_group_tiles(tr_scene *s, bool wait_for_setup)
{
    if (s->group_submitted == s->group_seq) return TR_OK;
    const PipelineDesc &pd = kPipelines[s->pipeline];
    const uint32_t np = (uint32_t)pd.n_passes;
    tr_scene::GroupSet &gs = s->grp[s->group_submitted % GROUP_SETS];
    const uint32_t G = gs.frames, g = gs.g;
    const TileArgs *h_tile = reinterpret_cast<const TileArgs *>(gs.h_tables + (size_t)np * G * sizeof(SetupArgs));
    const TileArgs *d_tile = reinterpret_cast<const TileArgs *>(gs.d_tables + (size_t)np * G * sizeof(SetupArgs));
    s->group_submitted++;
    if (wait_for_setup) HIP_TRY(hipStreamWaitEvent(s->stream, gs.ev_setup, 0));
    bool interior = true;  // (every pass of the group)
    // (has the chain completed?  "no wait needed" alone does not say so: a chain on the main stream itself needs none either)
    const bool chain_done = !wait_for_setup && !gs.chain_on_main && hipEventQuery(gs.ev_setup) == hipSuccess;
    for (uint32_t pi = 0; pi < np; pi++) {
        const PassDesc &pass = pd.pass[pi];
        const TileArgs &ta0 = h_tile[(size_t)pi * G];
        const int tile_waves = gs.tile_waves[pi], shared = gs.shared[pi];
        const EventPair ep = timing_pair(s, pass.fs == FS_DEPTH ? K_TILE_DEPTH : K_TILE, g);
        // (the group's "tiles done" event rides on its last tile kernel's own completion signal: a separate record
        // is one more packet between this group's tile kernel and the next one's)
        const bool last = pi + 1u == np;
        // Workgroups per frame: exactly the pass's work units when its chain has completed (the host has seen the event:
        // the lists' lengths are in page-locked memory), else one per tile
        const uint32_t units = (chain_done && use_work_units()) ? group_units(s, gs, pi, ta0.frame.ntx * ta0.frame.nty) : 0u;
        int rc = launch_tile(tile_fs(s, pass.fs), ta0, tile_waves, shared, gs.n_poly, d_tile + (size_t)pi * G, g, s->stream, ep.a,
                             (!s->profiling && last) ? gs.ev_tile : ep.b, units);
        if (rc) {
            s->broken = true;  // (the group's chains have run: counters not zeroed, ranges never consumed)
            return launch_status(rc, "k_tile");
        }
        if (s->profiling) s->events.push_back(ep);
        interior = interior && tile_launch_is_interior(tile_fs(s, pass.fs), ta0, tile_waves, shared, gs.n_poly, true);
    }
    s->fused_interior = interior ? 1 : 0;
    if (s->profiling) HIP_TRY(hipEventRecord(gs.ev_tile, s->stream));
    s->groups_unfenced = true;
    if (!s->own_stream) s->observed_seq = s->pass_seq;  // a caller's stream: handed on (see recover_from_overflow)
    return TR_OK;
}

// Hands groups to the main stream, oldest first.  As with single frames ("Handing tile kernels to the main
// stream" above) a cross-stream wait packet between two tile kernels costs microseconds and is not needed
// when the setup has already completed, so inside a long call a group's tile kernels go out one or two
// groups after its setup was queued -- by then the setup stream, which runs in the gaps and tails of the tile
// kernels before, has finished it.  `all`: the end of a call -- everything goes out, behind a wait if need be.
int submit_groups(tr_scene *s, bool all)
{
    int status = TR_OK;
    while (s->group_submitted < s->group_seq) {
        tr_scene::GroupSet &gs = s->grp[s->group_submitted % GROUP_SETS];
        bool ready = gs.chain_on_main || hipEventQuery(gs.ev_setup) == hipSuccess;  // (in order on the main stream: as good as done)
        if (!ready) {
            // a main stream that has run dry (the first group of a call, typically) gets the group at once, behind
            // a wait: an idle GPU loses nothing to the packet, and a call of a few frames is mostly start-up
            // (20 frames at 4096^2: 40.3 -> 33 us per frame)
            const bool idle = s->group_submitted == 0 ||
                              hipEventQuery(s->grp[(s->group_submitted - 1) % GROUP_SETS].ev_tile) == hipSuccess;
            // otherwise two groups are held back at most: the next setup needs the set of group_seq - GROUP_SETS,
            // whose tile kernels must be on the stream by then
            if (!all && !idle && s->group_seq - s->group_submitted <= 2) break;
            // It has to go now (the end of a call, or the host is about to sleep until a set is free).  While the main
            // stream still has a tile kernel to run, the chain -- which runs beside that kernel and is far shorter --
            // completes first: the HOST waits for it instead of a wait packet, and then knows the lists' lengths, i.e.
            // how many workgroups the tile kernel really needs (group_units: a third of the tiles at 4096^2).
            if (!idle && s->own_stream && use_work_units()) {
                HIP_TRY(hipEventSynchronize(gs.ev_setup));
                ready = true;
            }
        }
        int st = submit_group_tiles(s, !ready);
        if (st != TR_OK && status == TR_OK) status = st;
    }
    return status;
}

// All groups' tile kernels to the main stream, and -- once per batch of groups -- the setup stream ordered
// behind them: per-frame passes set up later reuse the per-frame bins and counters, which tile kernels queued
// so far may still read.
int finish_groups(tr_scene *s)
{
    int st = submit_groups(s, true);
    if (st != TR_OK) return st;
    if (s->groups_unfenced) {
        const tr_scene::GroupSet &gs = s->grp[(s->group_submitted + GROUP_SETS - 1) % GROUP_SETS];
        HIP_TRY(hipStreamWaitEvent(s->setup_stream, gs.ev_tile, 0));
        HIP_TRY(hipStreamWaitEvent(s->setup_stream2, gs.ev_tile, 0));
        s->groups_unfenced = false;
    }
    return TR_OK;
}

// ---------------------------------------------------------------------------------------------
// Automatic frame groups
// ---------------------------------------------------------------------------------------------
// The reference's caller renders frame after frame through clear -> set_* -> render (app.rs:170-213).  On the
// library's own stream nobody can observe a frame before the next getter / sync / flush, so `render` of a
// CLEARED frame only records the frame (light, camera, colour target) and returns; when a group's worth of
// frames has been recorded -- or anything needs them -- they are rendered together by the fused launches of
// run_group: the last one into the scene's current targets, the ones before it (which the per-frame protocol
// overwrites unobserved) into other frame slots.  A frame that must be seen alone (a getter right after it)
// goes through the ordinary per-frame path, so an interactive loop is what it was; a loop that keeps
// rendering gets the group rate without calling tr_scene_render_frames (4096^2 phong: 36 -> 30 us per frame).
// Not on a caller's stream (its next operation may consume the frame), not for accumulating renders, not with
// the winner tap or tile stamps (single buffers).  TR_OPT_NO_AUTO_GROUP / TR_AUTO_GROUP=0 turn it off.
bool frame_is_groupable(const tr_scene *s)
{
    static const int env_on = getenv("TR_AUTO_GROUP") ? atoi(getenv("TR_AUTO_GROUP")) : 1;
    return env_on && s->auto_group && s->own_stream && !s->d_winner && !s->d_stamps && s->z_fb_cleared &&
           (kPipelines[s->pipeline].n_passes == 1 || s->shadow_cleared) && group_size(s) > 1u;
}

// Renders the frames `render` has held back.  hold_back: a group has just filled up inside a running loop --
// its tile kernels may wait on the host until their setup has completed (submit_groups); otherwise everything
// is handed to the device now.
int flush_deferred(tr_scene *s, bool hold_back)
{
    if (!hold_back) s->auto_streak = 0;
    if (s->deferred.empty()) return TR_OK;
    std::vector<tr_scene::DeferredFrame> fr;
    fr.swap(s->deferred);
    const uint32_t g = (uint32_t)fr.size();
    int st = TR_OK;
    if (g == 1u) {
        // alone: the ordinary path, from the state the frame was recorded in
        const DrawState now(s);
        const bool z_now = s->z_fb_cleared, sh_now = s->shadow_cleared;
        uint8_t *fb_now = s->d_fb;
        s->view = fr[0].p;
        use_inst(s, fr[0].inst);
        s->z_fb_cleared = s->shadow_cleared = true;
        if (fr[0].fb != fb_now) st = use_slot(s, s->cur_slot, fr[0].fb == s->slots[(size_t)s->cur_slot].fb ? nullptr : fr[0].fb);
        if (st == TR_OK) st = render_frame(s);
        if (fr[0].fb != fb_now) {
            int st2 = use_slot(s, s->cur_slot, fb_now == s->slots[(size_t)s->cur_slot].fb ? nullptr : fb_now);
            if (st == TR_OK) st = st2;
        }
        // a clear() issued after that render stays pending
        s->z_fb_cleared = s->z_fb_cleared || z_now;
        s->shadow_cleared = s->shadow_cleared || sh_now;
        return st;
    }
    // per-frame tile kernels issued before these frames go first (same targets)
    st = submit_pending_tiles(s);
    if (st != TR_OK) return st;
    const uint32_t G = group_size(s);
    if (hold_back && (st = prepare_long_runs(s, true)) != TR_OK) return st;  // (a loop that fills groups: see there)
    if ((st = ensure_slots(s, G < g ? g : G)) != TR_OK) return st;
    tr_frame_params params[GROUP_MAX];
    tr_scene::InstRef insts[GROUP_MAX];
    void *fbs[GROUP_MAX];
    int slot_of[GROUP_MAX];
    std::vector<const void *> wanted(g);
    for (uint32_t j = 0; j < g; j++) {
        params[j] = fr[j].p;
        insts[j] = fr[j].inst;
        wanted[j] = fr[j].fb;
    }
    // which slot and which colour target every frame gets (tr_plan.h, plan_deferred): the last one the current targets,
    // the others -- which the per-frame protocol overwrites unobserved -- other slots
    const std::vector<plan::DeferredTarget> targets = plan::plan_deferred(
        wanted, s->cur_slot, s->slots[(size_t)s->cur_slot].fb, [s](const void *fb) { return own_frame_buffer(s, (const uint8_t *)fb); });
    for (uint32_t j = 0; j < g; j++) {
        slot_of[j] = targets[j].slot;
        fbs[j] = const_cast<void *>(targets[j].fb);
        // (such a frame can be seen in its buffer but not rendered again: only the last frame is replayed)
        if (targets[j].unreplayable)
            s->unreplayable_seq = s->pass_seq + (uint64_t)(j + 1u) * (uint64_t)kPipelines[s->pipeline].n_passes;
    }
    st = run_group(s, params, insts, fbs, slot_of, g);
    if (st == TR_OK) st = hold_back ? submit_groups(s, false) : finish_groups(s);
    return st;
}

// n cleared frames, frame i into slot i % G, drawing instance table insts[i] (insts == null: the current one);
// afterwards the last one is the scene's current frame.  posed: frame i draws a pose of its own -- POSED_WEIGHTS: weights
// pose_v + i * n_targets with the current palette, POSED_PALETTES: palette pose_v + i * n_bones * INST_XFORM_FLOATS with
// the current weights (pose_v null: without that half) -- made when its group is set up, so that only what holds a frame
// (its slot, the kept frames, work in flight) holds a pose's rows: not the call.
enum PerFramePose { POSED_NONE = 0, POSED_WEIGHTS, POSED_PALETTES };
int render_frames(tr_scene *s, uint32_t n, const tr_frame_params *p, const tr_scene::InstRef *insts, void *const *fbs,
                  PerFramePose posed = POSED_NONE, const float *pose_v = nullptr)
{
    int st = submit_pending(s);  // per-frame renders issued before go first
    if (st != TR_OK) return st;
    const uint32_t G = group_size(s);
    const uint32_t np = (uint32_t)kPipelines[s->pipeline].n_passes;
    // The groups of the call, its frame slots, what every group set must hold (tr_plan.h, plan_call): a long call's
    // groups grow, a short call's double from the usual one.
    static const uint32_t growth = (uint32_t)(getenv("TR_GROUP_GROWTH") ? atoi(getenv("TR_GROUP_GROWTH")) : 4);      // experiment hooks
    static const uint32_t short_factor = (uint32_t)(getenv("TR_SHORT_GROUPS") ? atoi(getenv("TR_SHORT_GROUPS")) : 3);  // (plan_call clamps them)
    const bool automatic = !s->d_winner && !s->d_stamps && !s->frames_per_launch && !getenv("TR_GROUP");
    const plan::CallPlan cp = plan::plan_call(n, G, long_run_group_size(s), automatic, (int)growth < 2 ? 2u : growth,
                                              (int)short_factor < 1 ? 1u : short_factor);
    const std::vector<uint32_t> &sizes = cp.sizes;
    const uint32_t S = cp.slots;
    if (n > G && (st = prepare_long_runs(s, fbs == nullptr)) != TR_OK) return st;
    if ((st = ensure_slots(s, S)) != TR_OK) return st;
    // all the sets of groups in flight now (allocations of a few hundred MiB each: not in the middle of a call)
    for (int k = 0; k < GROUP_SETS && !s->d_winner; k++)
        if ((st = ensure_group_set(s, s->grp[k], cp.set_frames)) != TR_OK) return st;
    s->host_status = TR_OK;
    const uint64_t first_seq = s->pass_seq;
    const uint32_t kept = cp.kept;  // what is left of the call: its last min(n, G) frames
    const bool per_frame = insts != nullptr || posed != POSED_NONE;
    std::vector<tr_scene::InstRef> kept_refs;  // their tables and poses
    const std::shared_ptr<tr_scene::Pose> pose0 = s->inst.pose;  // (its other half goes into every frame's pose)
    auto ref_of = [&](uint32_t i) {
        tr_scene::InstRef r = insts ? insts[i] : s->inst;
        if (posed == POSED_WEIGHTS)
            r.pose = make_pose(s, pose_v ? pose_v + (size_t)i * s->n_targets : nullptr, pose_palette(s, pose0));
        if (posed == POSED_PALETTES)
            r.pose = make_pose(s, pose_weights(s, pose0), pose_v ? pose_v + (size_t)i * s->n_bones * INST_XFORM_FLOATS : nullptr);
        if (i >= n - kept) kept_refs.push_back(r);
        return r;
    };
    if (s->d_winner) {
        // the winner tap is a single buffer: frame by frame through the ordinary path, slots all the same
        for (uint32_t i = 0; i < n; i++) {
            if ((st = use_slot(s, (int)(i % G), fbs ? (uint8_t *)fbs[i] : nullptr, fbs != nullptr)) != TR_OK) return st;
            s->view = p[i];
            if (per_frame) use_inst(s, ref_of(i));
            s->z_fb_cleared = s->shadow_cleared = true;
            if ((st = render_frame(s)) != TR_OK) return st;
        }
    } else {
        int slot_of[GROUP_MAX];
        tr_scene::InstRef refs[GROUP_MAX];  // the group's tables and poses (a pose per frame: made here, group by group)
        uint32_t i0 = 0;
        for (size_t k = 0; k < sizes.size(); i0 += sizes[k], k++) {
            const uint32_t g = sizes[k];
            for (uint32_t j = 0; j < g; j++) slot_of[j] = (int)((i0 + j) % S);
            for (uint32_t j = 0; j < g && per_frame; j++) refs[j] = ref_of(i0 + j);
            st = run_group(s, p + i0, per_frame ? refs : nullptr, fbs ? fbs + i0 : nullptr, slot_of, g,
                           fbs && !(s->flags & TR_OPT_TRUST_FRAME_BUFFERS));
            if (st == TR_OK) st = submit_groups(s, false);
            if (st != TR_OK) {
                // (a singular camera in frame i0 .. i0 + g - 1, or the device refused a launch): the groups before are
                // on their way, this one and the rest are not rendered; nothing of the call can be selected
                (void)finish_groups(s);
                s->host_status = st;
                s->tail.params.clear();
                s->tail.fbs.clear();
                s->tail.slot.clear();
                s->tail.inst.clear();
                s->last_was_group = true;
                s->last.valid = false;
                return st;
            }
        }
        if ((st = finish_groups(s)) != TR_OK) return st;
        // the scene now stands where the per-frame calls would have left it
        s->view = p[n - 1];
        if (per_frame) use_inst(s, kept_refs.back());
        s->z_fb_cleared = s->shadow_cleared = false;
        if ((st = use_slot(s, (int)((n - 1) % S), fbs ? (uint8_t *)fbs[n - 1] : nullptr)) != TR_OK) return st;
    }
    s->tail.params.assign(p + (n - kept), p + n);
    s->tail.fbs.clear();
    if (fbs) s->tail.fbs.assign(fbs + (n - kept), fbs + n);
    s->tail.slot.resize(kept);
    s->tail.inst.assign(kept, s->inst);
    if (per_frame) s->tail.inst = kept_refs;
    for (uint32_t k = 0; k < kept; k++) s->tail.slot[k] = (int)((n - kept + k) % (s->d_winner ? G : S));
    s->tail.first_seq = first_seq + (uint64_t)(n - kept) * np;
    if (fbs && n > kept) s->unreplayable_seq = s->tail.first_seq;  // older frames' buffers: theirs for good
    s->last_was_group = true;
    s->last.valid = false;
    if (s->pose_free.size() > POSE_FREE_MAX) trim_pose_pool(s, POSE_FREE_MAX);
    return TR_OK;
}

// After a bin overflow: the frames of the last call that still exist, again (the bins have grown).
int replay_tail(tr_scene *s)
{
    const uint32_t kept = (uint32_t)s->tail.params.size();
    if (kept == 0) return TR_OK;
    const int cur = s->cur_slot;
    uint8_t *cur_fb = s->d_fb;
    const DrawState now(s);
    int st = TR_OK;
    if (s->d_winner) {
        for (uint32_t k = 0; k < kept && st == TR_OK; k++) {
            st = use_slot(s, s->tail.slot[k], s->tail.fbs.empty() ? nullptr : (uint8_t *)s->tail.fbs[k]);
            s->view = s->tail.params[k];
            use_inst(s, s->tail.inst[k]);
            s->z_fb_cleared = s->shadow_cleared = true;
            if (st == TR_OK) st = render_frame(s);
        }
    } else {
        st = run_group(s, s->tail.params.data(), s->tail.inst.data(), s->tail.fbs.empty() ? nullptr : s->tail.fbs.data(),
                       s->tail.slot.data(), kept);
        if (st == TR_OK) st = finish_groups(s);
    }
    if (st != TR_OK) return st;
    return use_slot(s, cur, cur_fb == s->slots[(size_t)cur].fb ? nullptr : cur_fb);  // the selection the caller had
}

int find_pipeline(const char *name)
{
    if (!name) return -1;
    if (!strcmp(name, "true_normal")) name = "normal_map";  // README.md:18 spelling
    for (int i = 0; i < P_COUNT; i++)
        if (!strcmp(name, kPipelines[i].name)) return i;
    return -1;
}

// Records in a pass's pool for `n_poly` polygons: tr_options.bin_capacity, or 0 = automatic -- twice an estimate from
// the frame and the polygon count: a model that fills half the frame with half of its polygons facing the viewer has
// polygons with boxes of side s = sqrt(2 W H / n), each meeting (1 + s/128)(1 + s/16) tiles of 128x16: 5.0 pairs
// per polygon for the reference's model at 4096^2 (measured 2.4), 1.32 for its 8x8 grid at 8192^2 (measured
// 1.29) -- at least 65 536 records (6 MiB) and at most 16 Mi; a pass that wants more makes the pools grow (and is
// rendered again)
uint32_t pool_cap_for(uint32_t width, uint32_t height, uint64_t n_poly, uint64_t bin_capacity)
{
    uint64_t cap = bin_capacity;
    if (!cap) {
        const double n = (double)(n_poly ? n_poly : 1u);
        const double side = sqrt(2.0 * (double)width * (double)height / n);
        const double pairs = 0.5 * (1.0 + side / (double)TILE_W) * (1.0 + side / (double)TILE_H) * n;
        cap = (uint64_t)(2.0 * pairs);
        cap = cap < 65536u ? 65536u : cap > (16u << 20) ? (16u << 20) : cap;
    }
    if (cap < 64) cap = 64;
    if (cap > 0x7FFFFFFFull) cap = 0x7FFFFFFFull;
    return (uint32_t)cap;
}

// Everything the scene has been asked to render goes to the device and runs: afterwards nothing queued reads an array
// of the scene's, which may then be freed or replaced.
int drain(tr_scene *s)
{
    int st = submit_pending(s);
    if (st != TR_OK) return st;
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipStreamSynchronize(s->setup_stream));
    HIP_TRY(hipStreamSynchronize(s->setup_stream2));
    return TR_OK;
}

// Replaces the device array `d` by the `count` elements at `h` (`present` false: drops it).  The new array is allocated
// first; frames issued so far keep the old one -- everything queued runs (drain) before the scene changes hands.  A
// failure frees the new array and leaves the old one in place.
template <typename T>
int swap_device_array(tr_scene *s, T *&d, bool present, const T *h, size_t count)
{
    T *d_new = nullptr;
    int st = TR_OK;
    if (present && (st = dev_alloc(&d_new, count)) != TR_OK) return st;
    st = [&]() -> int {
        int rc = drain(s);
        if (rc != TR_OK) return rc;
        if (present) HIP_TRY(hipMemcpy(d_new, h, count * sizeof(T), hipMemcpyHostToDevice));
        HIP_TRY(hipStreamSynchronize(nullptr));  // (the scene's streams do not wait for the null stream)
        return TR_OK;
    }();
    if (st != TR_OK) {
        dev_free(d_new);
        return st;
    }
    dev_free(d);
    d = d_new;
    return TR_OK;
}

// A table of n instances is about to be drawn: the per-pass record arrays and (automatic bin capacity) the pools grow to
// what tr_scene_create gives the mesh replicated n times.  Never shrinks.  Waits for the scene's queued work when
// something grows (a new, larger table: not the steady state).
int grow_for_instances(tr_scene *s, uint32_t n)
{
    const uint64_t polys = (uint64_t)s->n_rows * (n ? n : 1u);
    const uint32_t cap = s->auto_bin_cap ? pool_cap_for(s->width, s->height, polys, 0) : s->pool_cap;
    if (polys <= s->poly_cap && cap <= s->pool_cap) return TR_OK;
    int st = drain(s);
    if (st != TR_OK) return st;
    for (tr_scene::GroupSet &gs : s->grp) gs.in_flight = false;  // (their tile kernels have run)
    if (polys > s->poly_cap) {
        s->poly_cap = polys;
        for (int k = 0; k < LOOKAHEAD; k++) {
            dev_free(s->d_recs[k]);
            if ((st = dev_alloc(&s->d_recs[k], (size_t)polys * s->rec_pieces))) return st;
        }
        for (tr_scene::GroupSet &gs : s->grp) free_group_set(gs);  // (allocated again, larger, when next used)
    }
    if (cap > s->pool_cap) {
        s->pool_cap = cap;
        for (int k = 0; k < LOOKAHEAD; k++) {
            dev_free(s->d_bins[k]);
            if ((st = dev_alloc(&s->d_bins[k], (size_t)s->pool_cap * s->rec_pieces))) return st;
        }
        // (the frame groups' bins follow pool_cap when their set is next used)
    }
    return TR_OK;
}

// tr_scene_set_instances / tr_scene_render_frames_instanced: n == 0 is "no table".
int check_instances(const tr_scene *s, uint32_t n, const void *inst)
{
    if (n && !inst) return tr::fail(TR_E_INVALID, "null instance table");
    if ((uint64_t)s->n_rows * n >= 0xFFFFFFF0ull) return tr::fail(TR_E_INVALID, "too many polygons (mesh polygons x instances)");
    return TR_OK;
}

// The posed calls' counts (tr_scene_set_morph_weights / _bone_palette and their render_frames forms): 0 is "none".
int check_weight_count(const tr_scene *s, uint32_t n)
{
    if (n != 0u && n != s->n_targets) return tr::fail(TR_E_INVALID, "n_weights must be 0 or the scene's number of morph targets");
    return TR_OK;
}

int check_bone_count(const tr_scene *s, uint32_t n)
{
    if (n != 0u && n != s->n_bones) return tr::fail(TR_E_INVALID, "n_bones must be 0 or the bone count of the scene's skin");
    return TR_OK;
}

void destroy(tr_scene *s)
{
    if (!s) return;
    (void)hipSetDevice(s->device);
    (void)submit_pending(s);
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    for (const EventPair &ep : s->events) {
        (void)hipEventDestroy(ep.a);
        (void)hipEventDestroy(ep.b);
    }
    for (hipEvent_t e : s->event_pool) (void)hipEventDestroy(e);
    dev_free(s->d_tri);
    if (s->setup_stream) (void)hipStreamSynchronize(s->setup_stream);
    if (s->setup_stream2) (void)hipStreamSynchronize(s->setup_stream2);
    for (const std::shared_ptr<tr_scene::InstBlock> &b : s->inst_blocks) free_inst_block(*b);
    s->inst_blocks.clear();
    // poses: every holder lets go, their rows come back to the pool, the pool goes
    s->inst = tr_scene::InstRef();
    s->last.inst = tr_scene::InstRef();
    s->deferred.clear();
    s->tail.inst.clear();
    for (tr_scene::FrameSlot &fs : s->slots) fs.z_inst = tr_scene::InstRef();
    for (tr_scene::PoseRows &r : s->pose_free) dev_free(r.d);
    s->pose_free.clear();
    s->pose_rows_live = 0;
    dev_free(s->d_delta);
    dev_free(s->d_skin);
    for (tr_scene::MorphStage *ring : { s->morph_stage, s->skin_stage })
        for (int k = 0; k < 4; k++) {
            tr_scene::MorphStage &m = ring[k];
            if (m.h) (void)hipHostFree(m.h);
            dev_free(m.d);
            m.done.reset();
        }
    for (int k = 0; k < 4; k++) dev_free(s->d_texel[k]);
    dev_free(s->d_packed);
    for (tr_scene::TexStage &t : s->tex_stage) {
        dev_free(t.d);
        if (t.done) (void)hipEventDestroy(t.done);
    }
    if (s->ev_tex) (void)hipEventDestroy(s->ev_tex);
    if (s->upload_stream) (void)hipStreamDestroy(s->upload_stream);
    for (int k = 0; k < LOOKAHEAD; k++) dev_free(s->d_lit[k]);
    if (s->setup_stream) (void)hipStreamSynchronize(s->setup_stream);
    if (s->setup_stream2) (void)hipStreamSynchronize(s->setup_stream2);
    for (int k = 0; k < RING; k++) {
        if (s->ev_setup[k]) (void)hipEventDestroy(s->ev_setup[k]);
        if (s->ev_tile[k]) (void)hipEventDestroy(s->ev_tile[k]);
    }
    if (s->ev_comp_ready) (void)hipEventDestroy(s->ev_comp_ready);
    if (s->ev_comp_done) (void)hipEventDestroy(s->ev_comp_done);
    if (s->setup_stream) (void)hipStreamDestroy(s->setup_stream);
    if (s->setup_stream2) (void)hipStreamDestroy(s->setup_stream2);
    for (tr_scene::BinState *b : { &s->bin_color, &s->bin_depth }) {
        for (int k = 0; k < SETS; k++) {
            dev_free(b->count[k]);
        }
    }
    for (int k = 0; k < LOOKAHEAD; k++) {
        dev_free(s->d_order[k]);
        dev_free(s->d_bins[k]);
        dev_free(s->d_recs[k]);
    }
    dev_free(s->d_bin_need);
    dev_free(s->d_overflow_seq);
    for (size_t k = s->slots.size(); k-- > 0;) {  // slot 0 last: the others may share its shadow buffer
        tr_scene::FrameSlot &fs = s->slots[k];
        dev_free(fs.z);
        dev_free(fs.zclean);
        if (k == 0 || fs.shadow != s->slots[0].shadow) {
            dev_free(fs.shadow);
            dev_free(fs.sclean);
        }
        dev_free(fs.fb);
    }
    for (tr_scene::GroupSet &g : s->grp) {
        dev_free(g.bins);
        dev_free(g.recs);
        dev_free(g.lit);
        dev_free(g.count);
        dev_free(g.order);
        dev_free(g.d_tables);
        if (g.h_tables) (void)hipHostFree(g.h_tables);
        if (g.ev_setup) (void)hipEventDestroy(g.ev_setup);
        if (g.ev_tile) (void)hipEventDestroy(g.ev_tile);
    }
    dev_free(s->d_view);
    dev_free(s->d_resolved);
    dev_free(s->d_dof_fb);
    dev_free(s->d_dof_clean);
    dev_free(s->d_lut);
    dev_free(s->d_ramp);
    dev_free(s->d_dist_mask);
    dev_free(s->d_dist_h);
    dev_free(s->d_dist_summary);
    dev_free(s->d_dist_field);
    dev_free(s->d_lines);
    dev_free(s->resize.d);
    if (s->resize.h) (void)hipHostFree(s->resize.h);
    if (s->resize.uploaded) (void)hipEventDestroy(s->resize.uploaded);
    dev_free(s->warp.d);
    if (s->warp.h) (void)hipHostFree(s->warp.h);
    if (s->warp.uploaded) (void)hipEventDestroy(s->warp.uploaded);
    dev_free(s->d_stats_partials);
    dev_free(s->d_winner);
    for (tr_scene::FbFlags &f : s->fb_flags) dev_free(f.clean);
    for (tr_scene::HostFlags &f : s->host_flags) dev_free(f.clean);
    dev_free(s->d_stamps);
    dev_free(s->d_err);
    if (s->h_alarm) (void)hipHostFree((void *)s->h_alarm);
    if (s->own_stream && s->stream) (void)hipStreamDestroy(s->stream);
    delete s;
}

int create(uint32_t width, uint32_t height, const tr_mesh *mesh, const tr_image_rgb8 tex[4],
           const char *pipeline_name, const tr_options *opts, tr_scene *s)
{
    const int pipe = find_pipeline(pipeline_name);
    if (pipe < 0) return tr::fail(TR_E_UNKNOWN_PIPELINE, "Provided pipeline name is not supported!");
    if (width == 0 || height == 0 || width > 32768u || height > 32768u)
        return tr::fail(TR_E_INVALID, "frame size must be within 1..32768");
    if (!mesh || !tex) return tr::fail(TR_E_INVALID, "null mesh or textures");
    if (mesh->n_tri >= 0xFFFFFFF0u) return tr::fail(TR_E_INVALID, "too many polygons");
    for (uint32_t t = 0; t < mesh->n_tri; t++) {
        const uint32_t *ix = mesh->idx + 9u * (size_t)t;
        for (int k = 0; k < 3; k++)
            if (ix[3 * k] >= mesh->n_pos || ix[3 * k + 1] >= mesh->n_tex || ix[3 * k + 2] >= mesh->n_nrm)
                return tr::fail(TR_E_BAD_POLYGON, "polygon index outside positions / tex_coords / normals");
    }
    for (int k = 0; k < 4; k++)
        if (!tex[k].rgb || tex[k].w == 0 || tex[k].h == 0 || tex[k].w > 65535u || tex[k].h > 65535u)
            return tr::fail(TR_E_INVALID, "texture must be non-empty and at most 65535 on a side");

    tr_options o;
    memset(&o, 0, sizeof o);
    o.device = -1;
    if (opts) memcpy(&o, opts, opts->struct_size < sizeof o ? opts->struct_size : sizeof o);

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return tr::fail(TR_E_HIP, "no HIP device available (this library has no CPU rendering path)");
    int dev = o.device;
    if (dev < 0) HIP_TRY(hipGetDevice(&dev));
    if (dev >= ndev) return tr::fail(TR_E_INVALID, "device ordinal out of range");
    HIP_TRY(hipSetDevice(dev));
    s->device = dev;
    s->width = width;
    s->height = height;
    s->pipeline = pipe;
    s->flags = o.flags;
    if (o.tile_waves != 0 && o.tile_waves != 4 && o.tile_waves != 8 && o.tile_waves != 16)
        return tr::fail(TR_E_INVALID, "tile_waves must be 0, 4, 8 or 16");
    s->tile_waves = o.tile_waves;
    if (o.tile_mode > 2) return tr::fail(TR_E_INVALID, "tile_mode must be 0 (automatic), 1 (columns) or 2 (shared bin)");
    s->tile_mode = o.tile_mode;
    if (o.frames_per_launch > (uint32_t)GROUP_MAX) return tr::fail(TR_E_INVALID, "frames_per_launch must be 0 (automatic) or 1..32");
    s->frames_per_launch = o.frames_per_launch;
    if (o.max_frame_slots > (uint32_t)GROUP_MAX) return tr::fail(TR_E_INVALID, "max_frame_slots must be 0 (automatic) or 1..32");
    if (o.max_frame_slots && o.frames_per_launch > o.max_frame_slots)
        return tr::fail(TR_E_INVALID, "frames_per_launch exceeds max_frame_slots (every frame of a launch needs a slot)");
    s->max_slots = o.max_frame_slots;
    s->auto_group = (o.flags & TR_OPT_NO_AUTO_GROUP) == 0;
    s->transient_depth = (o.flags & TR_OPT_STORE_DEPTH) == 0;

    if (o.stream) {
        s->stream = (hipStream_t)o.stream;
    } else {
        HIP_TRY(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
        s->own_stream = true;
    }

    // band (output rows, row 0 = top) -> internal rows (row 0 = bottom)
    uint32_t r0 = o.band_row0, r1 = o.band_row1;
    if (r0 == 0 && r1 == 0) r1 = height;
    if (r0 >= r1 || r1 > height) return tr::fail(TR_E_INVALID, "band rows must satisfy row0 < row1 <= height");
    s->frame.width = width;
    s->frame.height = height;
    s->frame.band_y0 = (int32_t)(height - r1);
    s->frame.band_y1 = (int32_t)(height - r0);
    s->frame.ntx = (width + TILE_W - 1) / TILE_W;
    s->frame.ty_base = s->frame.band_y0 / TILE_H;
    s->frame.nty = (uint32_t)((s->frame.band_y1 - 1) / TILE_H - s->frame.ty_base + 1);
    s->n_tiles = s->frame.ntx * s->frame.nty;
    s->frame_full = s->frame;
    s->frame_full.band_y0 = 0;
    s->frame_full.band_y1 = (int32_t)height;
    s->frame_full.ty_base = 0;
    s->frame_full.nty = (height + TILE_H - 1) / TILE_H;
    s->n_tiles_full = s->frame_full.ntx * s->frame_full.nty;

    const size_t npx = (size_t)width * height;
    int st;
    // model: one flat row per polygon
    {
        std::vector<float> rows((size_t)mesh->n_tri * TRI_FLOATS);
        for (uint32_t t = 0; t < mesh->n_tri; t++)
            gather_polygon(mesh->pos, mesh->tex, mesh->nrm, mesh->idx + 9u * (size_t)t, &rows[(size_t)t * TRI_FLOATS]);
        if ((st = dev_alloc(&s->d_tri, rows.size()))) return st;
        HIP_TRY(hipMemcpy(s->d_tri, rows.data(), rows.size() * 4, hipMemcpyHostToDevice));
    }
    s->n_rows = mesh->n_tri;
    s->mesh_idx.assign(mesh->idx, mesh->idx + 9u * (size_t)mesh->n_tri);  // (for the gather of morph targets)
    s->n_pos = mesh->n_pos;
    s->n_nrm = mesh->n_nrm;
    s->poly_cap = mesh->n_tri;
    use_inst(s, tr_scene::InstRef());

    // textures: rgb8 -> rgba8 so a texel is one aligned dword fetch
    std::vector<uint32_t> rgba[4];
    bool same_size = true;
    for (int k = 0; k < 4; k++) {
        const size_t n = (size_t)tex[k].w * tex[k].h;
        rgba[k].resize(n);
        for (size_t i = 0; i < n; i++)
            rgba[k][i] = (uint32_t)tex[k].rgb[3 * i] | ((uint32_t)tex[k].rgb[3 * i + 1] << 8) |
                         ((uint32_t)tex[k].rgb[3 * i + 2] << 16);
        if ((st = dev_alloc(&s->d_texel[k], n))) return st;
        HIP_TRY(hipMemcpy(s->d_texel[k], rgba[k].data(), n * 4, hipMemcpyHostToDevice));
        s->tex.texel[k] = s->d_texel[k];
        s->tex.w[k] = tex[k].w;
        s->tex.h[k] = tex[k].h;
        same_size = same_size && tex[k].w == tex[0].w && tex[k].h == tex[0].h;
    }
    // ... and, when they all have one size, the images the colour closure reads as ONE array: interleaved texel by
    // texel, tiled into 128-byte blocks (tr_texels.h; fetch_texels, tr_shaders.h)
    static const bool plain_texels = getenv("TR_PLAIN_TEXELS") && atoi(getenv("TR_PLAIN_TEXELS"));  // test hook
    if (same_size && !plain_texels) {
        const int fs = kPipelines[pipe].pass[kPipelines[pipe].n_passes - 1].fs;
        const uint32_t *const image[4] = { rgba[0].data(), rgba[1].data(), rgba[2].data(), rgba[3].data() };
        uint32_t bpr = 0;
        const std::vector<uint32_t> packed = pack_texels(fs, image, tex[0].w, tex[0].h, bpr);
        if ((st = dev_alloc(&s->d_packed, packed.size()))) return st;
        HIP_TRY(hipMemcpy(s->d_packed, packed.data(), packed.size() * 4, hipMemcpyHostToDevice));
        s->tex.packed = s->d_packed;
        s->tex.packed_bpr = bpr;
        s->packed_count = packed.size();
        s->set_fs = fs;
        // The lit path (k_lit): for the closures that are functions of the texel alone, when a frame has many more
        // pixels than the images have texels.  1 Mi texels cost 11 us (specular) / 8 us (normal map) per frame beside
        // the tile kernels; measured per frame, per-fragment -> lit: specular 4096^2 42.8 -> 34.5 us, x64 grid at 8192^2
        // 313 -> 223; normal map 4096^2 33.6 -> 32.7; at 2048^2 both lose (14.9 -> 16.3, 11.8 -> 13.6): from sixteen
        // pixels per texel.  (TR_LIT=0/1 overrides: tests run small frames through it.)
        if (fs == FS_NORMAL_MAP || fs == FS_SPECULAR) {
            const char *force = getenv("TR_LIT");
            const uint64_t texels = (uint64_t)tex[0].w * tex[0].h, pixels = (uint64_t)width * height;
            s->lit = force ? atoi(force) != 0 : pixels >= LIT_PIXELS_PER_TEXEL * texels;
            if (s->lit) {
                s->set_bpr = bpr;
                s->lit_bpr = (tex[0].w + 7u) / 8u;
                s->lit_words = s->lit_bpr * ((tex[0].h + 3u) / 4u) * 32u;
                for (int k = 0; k < LOOKAHEAD; k++)
                    if ((st = dev_alloc(&s->d_lit[k], (size_t)s->lit_words))) return st;
            }
        }
    }

    // bins
    for (tr_scene::BinState *b : { &s->bin_color, &s->bin_depth }) {
        const size_t nt = (b == &s->bin_color) ? s->n_tiles : s->n_tiles_full;
        for (int k = 0; k < SETS; k++) {
            // nt counters, then k_order's 8 bucket sizes and 8 cursors
            if ((st = dev_alloc(&b->count[k], nt + 16))) return st;
            HIP_TRY(hipMemset(b->count[k], 0, (nt + 16) * 4));
        }
    }
    for (int k = 0; k < LOOKAHEAD; k++)
        if ((st = dev_alloc(&s->d_order[k], (size_t)s->n_tiles_full * ORDER_LISTS))) return st;
    if ((st = dev_alloc(&s->d_bin_need, 1))) return st;
    // records in a pass's pool = all its (polygon, tile) pairs.  Automatic: twice an estimate from the frame and
    // the polygon count -- a model that fills half the frame with half of its polygons facing the viewer has
    // polygons with boxes of side s = sqrt(2 W H / n), each meeting (1 + s/128)(1 + s/16) tiles of 128x16: 5.0 pairs
    // per polygon for the reference's model at 4096^2 (measured 2.4), 1.32 for its 8x8 grid at 8192^2 (measured
    // 1.29) -- at least 65 536 records (6 MiB) and at most 16 Mi; a pass that wants more makes the pools grow (and is
    // rendered again)
    s->auto_bin_cap = o.bin_capacity == 0;
    s->pool_cap = pool_cap_for(width, height, mesh->n_tri, o.bin_capacity);
    s->rec_pieces = (pipe == P_DARBOUX) ? REC_PIECES_LARGE : REC_PIECES_SMALL;
    for (int k = 0; k < LOOKAHEAD; k++) {
        if ((st = dev_alloc(&s->d_bins[k], (size_t)s->pool_cap * s->rec_pieces))) return st;
        if ((st = dev_alloc(&s->d_recs[k], (size_t)(mesh->n_tri ? mesh->n_tri : 1u) * s->rec_pieces))) return st;
    }
    HIP_TRY(hipStreamCreateWithFlags(&s->setup_stream, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&s->setup_stream2, hipStreamNonBlocking));
    s->two_setup_streams = !(getenv("TR_SETUP_STREAMS") && atoi(getenv("TR_SETUP_STREAMS")) == 1);  // experiment hook
    for (int k = 0; k < RING; k++) {
        HIP_TRY(hipEventCreateWithFlags(&s->ev_setup[k], hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&s->ev_tile[k], hipEventDisableTiming));
    }
    HIP_TRY(hipMemset(s->d_bin_need, 0, 4));
    if ((st = dev_alloc(&s->d_overflow_seq, 1))) return st;
    HIP_TRY(hipMemset(s->d_overflow_seq, 0xFF, sizeof(unsigned long long)));

    // render targets; Buffer::new / Scene::new zero-fill them (shader.rs:46-47, scene.rs:71)
    s->slots.resize(1);
    {
        tr_scene::FrameSlot &fs = s->slots[0];
        if ((st = dev_alloc(&fs.z, npx))) return st;
        if ((st = dev_alloc(&fs.shadow, npx))) return st;
        HIP_TRY(hipMemset(fs.z, 0, npx * 4));
        HIP_TRY(hipMemset(fs.shadow, 0, npx * 4));
        if ((st = dev_alloc(&fs.zclean, (size_t)s->n_tiles))) return st;
        HIP_TRY(hipMemset(fs.zclean, 0, (size_t)s->n_tiles * 4));
        if ((st = dev_alloc(&fs.sclean, (size_t)s->n_tiles_full))) return st;
        HIP_TRY(hipMemset(fs.sclean, 0, (size_t)s->n_tiles_full * 4));
    }
    if (o.flags & TR_OPT_WINNER_TAP) {
        if ((st = dev_alloc(&s->d_winner, npx))) return st;
        HIP_TRY(hipMemset(s->d_winner, 0xFF, npx * 4));
    }
    if ((st = use_slot(s, 0, (uint8_t *)o.frame_buffer_device))) return st;
    if (s->d_fb == s->slots[0].fb)  // zero-filled just now, winner tap at "no fragment": every tile is clean
        HIP_TRY(hipMemsetAsync(s->d_fbclean, 0xFF, (size_t)s->n_tiles * 4, s->stream));
    if (o.flags & TR_OPT_TILE_STAMPS) {
        if ((st = dev_alloc(&s->d_stamps, (size_t)s->n_tiles_full * 8))) return st;
        HIP_TRY(hipMemset(s->d_stamps, 0, (size_t)s->n_tiles_full * 64));
    }
    if ((st = dev_alloc(&s->d_err, 1))) return st;
    HIP_TRY(hipMemset(s->d_err, 0, 4));
    {
        void *h = nullptr, *d = nullptr;
        HIP_TRY(hipHostMalloc(&h, 64, hipHostMallocMapped));
        HIP_TRY(hipHostGetDevicePointer(&d, h, 0));
        s->h_alarm = (volatile uint32_t *)h;
        s->d_alarm = (uint32_t *)d;
        *s->h_alarm = 0u;
    }
    HIP_TRY(hipDeviceSynchronize());
    return TR_OK;
}

// Getters run in this order: (1) wait for the frame and take its status -- a bin overflow found
// here grows the bins and renders the frame again; (2) only then enqueue what derives from the
// frame (a pending clear, the fast-clear flags' f32::MIN, the u8 depth view); (3) wait, copy.
// Deriving first would copy out a view of the truncated frame.  The frame's status is returned
// after the copy (TR_E_OOB_LOOKUP / TR_E_BIN_OVERFLOW frames are still delivered); TR_E_HIP ends
// the call.
bool fatal(int st) { return st == TR_E_HIP || st == TR_E_NOMEM || st == TR_E_INVALID; }

// Does the scene render the whole frame (no band, tr_options.band_row0/1)?
bool whole_frame(const tr_scene *s) { return s->frame.band_y0 == 0 && s->frame.band_y1 == (int32_t)s->height; }

// The refusal of every entry point that would queue work on a broken scene.
int unusable() { return tr::fail(TR_E_HIP, "the scene is unusable: a tile kernel could not be launched behind its chain"); }

// Every pass issued so far is now in a consumer's hands -- a copy, a stage or a merge has read the frame, or changed
// it: a bin overflow among those passes can no longer be repaired by rendering again (that would undo what was made in
// place, or change the frame that a result made elsewhere was made from), and tr_scene_sync will say so
// (TR_E_BIN_OVERFLOW).
void handed_on(tr_scene *s) { s->observed_seq = s->pass_seq; }

// tr_scene_resolve / tr_scene_get_resolved: is `factor` one this scene's frame can be resolved by?  (A source block
// of factor x factor pixels must not straddle a 128 x 16 tile or the scene's band.)
int check_resolve(const tr_scene *s, uint32_t factor)
{
    if (factor != 2u && factor != 4u && factor != 8u) return tr::fail(TR_E_INVALID, "resolve: the factor must be 2, 4 or 8");
    if (s->width % factor || s->height % factor)
        return tr::fail(TR_E_INVALID, "resolve: the frame's width and height must be multiples of the factor");
    if (s->frame.band_y0 % (int32_t)factor || s->frame.band_y1 % (int32_t)factor)
        return tr::fail(TR_E_INVALID, "resolve: the band's rows (tr_options.band_row0/1) must be multiples of the factor");
    return TR_OK;
}

size_t resolved_bytes(const tr_scene *s, uint32_t factor) { return (size_t)(s->width / factor) * (s->height / factor) * 3; }

// The tail of an enqueue_*: the launch inside its timing scope, a refusal under the kernel's name, the stream no longer idle.
template <typename Launch>
int timed_launch(tr_scene *s, int kernel, const char *name, Launch launch)
{
    {
        Timed t(s, kernel);
        int rc = launch();
        if (rc) return launch_status(rc, name);
    }
    s->quiescent = false;
    return TR_OK;
}

// Enqueues the resolve of the current frame into `out_device` behind everything issued so far.
int enqueue_resolve(tr_scene *s, uint32_t factor, uint8_t *out_device)
{
    int st = flush_clear_color(s);
    if (st != TR_OK) return st;
    st = submit_pending(s);
    if (st != TR_OK) return st;
    return timed_launch(s, K_RESOLVE, "k_resolve", [&] { return launch_resolve(s->d_fb, out_device, s->d_fbclean, s->frame, factor, s->stream); });
}

int finish_read_back(tr_scene *s, int frame_status, void *dst, const void *src, size_t bytes)
{
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return frame_status;
}

// ---------------------------------------------------------------------------------------------
// Stage entry points: what tr_scene_<stage>(.., out) and tr_scene_get_<stage>(.., rgb) share
// ---------------------------------------------------------------------------------------------
// A stage (resolve, accumulate, depth of field, bloom, grade, outline, antialias, warp, convolve, rank, bilateral, resize, to_yuv, layer, ramp, lines, distance, projector, relight) derives an image from the current frame.  Its own code is
// its checks and its enqueue_*; the rest is the helpers below, called in one order ("Adding a stage"):
//   tr_scene_<stage>: null scene; parameter checks; scene checks (band, table, unusable()); hipSetDevice; classify_out
//   for a non-null `out`, then refuse_overlap (resolve and resize have none; to_yuv has no in-place form either); the cleared-scene shortcut where the stage has one --
//   cleared_out_of_place, while in place a cleared frame is its own result and NOTHING happens, handed_on included; the
//   enqueue_* into the target, into the frame itself, or through the scratch frame (in_place_via_scratch); handed_on.
//   The frame-sized stages that go through the scratch frame (depth of field, bloom, antialias, convolve, rank, bilateral) call
//   scratch_stage after their checks: it is that order from hipSetDevice on.
//   tr_scene_get_<stage>: the same checks, then get_stage (those six: get_scratch_stage).
//   enqueue_*: the stage's queue choice; its arguments (frame_stage_args: the five fields every such kernel takes);
//   timed_launch -- the launch under Timed, launch_status under the kernel's name, quiescent = false.
// A refused call has queued nothing and changed nothing, but for the read-back record of a tr_host_alloc `out` that
// classify_out accepted.  In place a colour-clean flag of the DEVICE buffer may change; a record of a page-locked host
// buffer (HostFlags) says what that host buffer holds, which no in-place call changes: the next read-back compares the
// two as always.  Each enqueue_* keeps its own choice among flush_clear_color, submit_pending and depth_in_memory, written
// out in its own function ahead of the shared calls: that choice decides whether a depth left on the chip stays there.

size_t frame_bytes(const tr_scene *s) { return (size_t)s->width * s->height * 3; }

// The scene's rows of a frame-sized buffer: their first byte and their number of bytes (a whole frame: all of it).
void band_bytes(const tr_scene *s, size_t *first, size_t *count)
{
    *first = (size_t)s->width * (size_t)(s->height - (uint32_t)s->frame.band_y1) * 3;
    *count = (size_t)s->width * (size_t)(s->frame.band_y1 - s->frame.band_y0) * 3;
}

// The frame on its way, its depth in memory behind valid flags.
int depth_in_memory(tr_scene *s)
{
    int st = submit_pending(s);
    if (st == TR_OK) st = ensure_depth(s);
    if (st == TR_OK) st = need_z(s, s->cur_slot);
    return st;
}

// The colour buffer of the frame tr_scene_select_frame(s, back) would make current.
uint8_t *kept_frame_buffer(const tr_scene *s, uint32_t back)
{
    const size_t k = s->tail.params.size() - 1u - back;
    return s->tail.fbs.empty() ? s->slots[(size_t)s->tail.slot[k]].fb : (uint8_t *)s->tail.fbs[k];
}

// `out` of a stage: memory from tr_host_alloc of at least `bytes` bytes (the kernel stores through its mapped address,
// and the buffer's sparse read-back record lapses) or device memory.  The address the kernel stores to goes to *target.
// who / getter / frame: the entry point's words in the error texts.
int classify_out(void *out, size_t bytes, const char *who, const char *getter, const char *frame, void **target_out)
{
    const std::string w(who);
    void *target = nullptr;
    bool known_host = false;
    {
        std::lock_guard<std::mutex> lock(g_host_mutex);
        auto it = g_host_allocs.find(out);
        if (it != g_host_allocs.end()) {
            known_host = true;
            if (it->second.bytes >= bytes) {
                target = it->second.device;
                // (whatever a scene remembered of the buffer's zero tiles from a sparse read-back has lapsed)
                it->second.writer = 0u;
                it->second.gen += 1u;
            }
        }
    }
    if (known_host && !target) return tr::fail(TR_E_INVALID, w + ": the host buffer is smaller than the " + frame);
    if (!target) {
        const std::string text = w + ": `out` is neither device memory nor from tr_host_alloc (" + getter + " takes any host memory)";
        hipPointerAttribute_t attr = {};
        if (hipPointerGetAttributes(&attr, out) != hipSuccess) {
            (void)hipGetLastError();  // (ordinary host memory is an error to the runtime: not a sticky one)
            return tr::fail(TR_E_INVALID, text);
        }
        if (attr.type != hipMemoryTypeDevice) return tr::fail(TR_E_INVALID, text);
        target = out;
    }
    *target_out = target;
    return TR_OK;
}

// `target` (from classify_out) must not be (part of) a frame the kernel may read, or another one the scene keeps flags
// of: none of its slots, no frame buffer with a flag set, none of the last n_kept kept frames.  bytes: a frame's;
// target_bytes: the target's where it differs (0: the same).
int refuse_overlap(const tr_scene *s, const void *target, size_t bytes, const char *who, const char *verb, uint32_t n_kept,
                   size_t target_bytes = 0)
{
    if (target_bytes == 0u) target_bytes = bytes;
    auto overlaps = [&](const uint8_t *fb) {
        return fb && (const uint8_t *)target < fb + bytes && fb < (const uint8_t *)target + target_bytes;
    };
    bool hit = false;
    for (const tr_scene::FrameSlot &fs : s->slots) hit = hit || overlaps(fs.fb);
    for (const tr_scene::FbFlags &f : s->fb_flags) hit = hit || overlaps(f.fb);
    for (uint32_t k = 0; k < n_kept; k++) hit = hit || overlaps(kept_frame_buffer(s, k));
    if (!hit) return TR_OK;
    return tr::fail(TR_E_INVALID, std::string(who) + ": `out` overlaps a frame buffer of the scene (out == NULL " + verb + " in place)");
}

// A non-null `out` of a frame-sized stage through both steps; null (in place) leaves *target null.
int frame_out(const tr_scene *s, void *out, const char *who, const char *getter, const char *verb, uint32_t n_kept, void **target)
{
    *target = nullptr;
    if (!out) return TR_OK;
    int st = classify_out(out, frame_bytes(s), who, getter, "frame", target);
    return st != TR_OK ? st : refuse_overlap(s, *target, frame_bytes(s), who, verb, n_kept);
}

// The cleared-scene shortcut out of place: the stage's image of a logically cleared frame is black, so the scene's rows
// of `target` become zeros behind everything issued so far, and no kernel runs.
int cleared_out_of_place(tr_scene *s, void *target)
{
    int st = submit_pending(s);
    if (st != TR_OK) return st;
    size_t first = 0, count = 0;
    band_bytes(s, &first, &count);
    HIP_TRY(hipMemsetAsync((uint8_t *)target + first, 0, count, s->stream));
    s->quiescent = false;
    handed_on(s);
    return TR_OK;
}

// The frame, its flags and the output in a stage's kernel arguments (out_clean: null, or where the kernel writes the
// flags of `out_device`).
template <typename Args>
void frame_stage_args(Args &a, const tr_scene *s, uint8_t *out_device, uint32_t *out_clean)
{
    a.fb = s->d_fb;
    a.fbclean = s->d_fbclean;
    a.out = out_device;
    a.out_clean = out_clean;
    a.frame = s->frame;
}

// In place for a stage that reads neighbours: enqueue(out_device, out_clean) into the scene's scratch frame and flag
// set (one pair, shared: each call leaves them free behind its two copies), then, in stream order, the colour over the
// current frame and the flags over the frame's colour-clean flags.
template <typename Enqueue>
int in_place_via_scratch(tr_scene *s, Enqueue enqueue)
{
    int st = TR_OK;
    if (!s->d_dof_fb && (st = dev_alloc(&s->d_dof_fb, frame_bytes(s)))) return st;
    if (!s->d_dof_clean && (st = dev_alloc(&s->d_dof_clean, (size_t)s->n_tiles))) return st;
    if ((st = enqueue(s->d_dof_fb, s->d_dof_clean)) != TR_OK) return st;
    HIP_TRY(hipMemcpyAsync(s->d_fb, s->d_dof_fb, frame_bytes(s), hipMemcpyDeviceToDevice, s->stream));
    if (s->d_fbclean) HIP_TRY(hipMemcpyAsync(s->d_fbclean, s->d_dof_clean, (size_t)s->n_tiles * 4, hipMemcpyDeviceToDevice, s->stream));
    return TR_OK;
}

// tr_scene_<stage>(s, .., out) of a frame-sized stage that goes in place through the scratch frame, after the stage's
// checks.  who / getter / verb: the entry point's words in the error texts; black_stays_black: the stage's image of a
// black frame is black, so a logically cleared frame gives zeros out of place and is its own result in place;
// enqueue(out_device, out_clean): the stage's enqueue_*.
template <typename Enqueue>
int scratch_stage(tr_scene *s, void *out, const char *who, const char *getter, const char *verb, bool black_stays_black, Enqueue enqueue)
{
    HIP_TRY(hipSetDevice(s->device));
    void *target = nullptr;
    int st = frame_out(s, out, who, getter, verb, 0u, &target);
    if (st != TR_OK) return st;
    if (s->z_fb_cleared && black_stays_black) return target ? cleared_out_of_place(s, target) : TR_OK;
    st = target ? enqueue((uint8_t *)target, nullptr) : in_place_via_scratch(s, enqueue);
    if (st == TR_OK) handed_on(s);
    return st;
}

// The library's read-back buffer, one per scene and shared by every getter: s->d_resolved of at least `bytes` bytes,
// grown only while the stream is idle (sync_and_status has waited).  zero: the kernel will not cover all of it -- a band
// scene's writes its own rows only, a stage that short-circuits on a cleared scene runs none -- and the rest reads as zeros.
int read_back_buffer(tr_scene *s, size_t bytes, bool zero)
{
    if (s->resolved_bytes < bytes) {
        dev_free(s->d_resolved);
        s->resolved_bytes = 0;
        int st = dev_alloc(&s->d_resolved, bytes);
        if (st) return st;
        s->resolved_bytes = bytes;
    }
    if (zero) HIP_TRY(hipMemsetAsync(s->d_resolved, 0, bytes, s->stream));
    return TR_OK;
}

// Does a stage whose image of a black frame is black short-circuit?  (depth of field, bloom; grade: cleared_to_black)
bool cleared(const tr_scene *s) { return s->z_fb_cleared; }

// tr_scene_get_<stage>, after the stage's checks, in the getters' order (above): wait for the frame and take its status;
// enqueue(out_device) into the library's buffer -- unless the stage short-circuits on this scene (short_circuits, may be
// null; asked after the wait, which may have rendered held-back frames) --; wait, copy `bytes` bytes to rgb.
template <typename Enqueue>
int get_stage(tr_scene *s, uint8_t *rgb, size_t bytes, bool (*short_circuits)(const tr_scene *), Enqueue enqueue)
{
    int fst = sync_and_status(s);
    if (fatal(fst)) return fst;
    const bool skip = short_circuits && short_circuits(s);
    int st = read_back_buffer(s, bytes, skip || !whole_frame(s));
    if (st == TR_OK && !skip) st = enqueue(s->d_resolved);
    if (st != TR_OK) return st;
    return finish_read_back(s, fst, rgb, s->d_resolved, bytes);
}

// tr_scene_get_<stage> of the stages of scratch_stage, after the stage's checks: the same black_stays_black and enqueue.
template <typename Enqueue>
int get_scratch_stage(tr_scene *s, uint8_t *rgb, bool black_stays_black, Enqueue enqueue)
{
    return get_stage(s, rgb, frame_bytes(s), black_stays_black ? cleared : nullptr, [&](uint8_t *o) { return enqueue(o, nullptr); });
}

// A launch on dst's stream that reads src's buffers and writes dst's: behind src's work, and src's stream behind the
// launch, so that a later render of src does not overtake it.  Both scenes' passes are then handed on: rendering one of
// them again after a bin overflow would undo the merge, or change what it read.
template <typename Launch>
int cross_scene_launch(tr_scene *dst, tr_scene *src, Launch launch)
{
    if (!src->ev_comp_ready) HIP_TRY(hipEventCreateWithFlags(&src->ev_comp_ready, hipEventDisableTiming));
    if (!dst->ev_comp_done) HIP_TRY(hipEventCreateWithFlags(&dst->ev_comp_done, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(src->ev_comp_ready, src->stream));
    HIP_TRY(hipStreamWaitEvent(dst->stream, src->ev_comp_ready, 0));
    int st = launch();
    if (st != TR_OK) return st;
    HIP_TRY(hipEventRecord(dst->ev_comp_done, dst->stream));
    HIP_TRY(hipStreamWaitEvent(src->stream, dst->ev_comp_done, 0));
    dst->quiescent = src->quiescent = false;
    handed_on(dst);
    handed_on(src);
    return TR_OK;
}

int depth_view(tr_scene *s, int frame_status, const float *src, uint8_t *rgb)
{
    const size_t npx = (size_t)s->width * s->height;
    if (!s->d_view) {
        int st = dev_alloc(&s->d_view, npx * 3);
        if (st) return st;
    }
    int rc = launch_depth_view(src, s->d_view, s->width, s->height, s->stream);
    if (rc) return launch_status(rc, "k_depth_view");
    return finish_read_back(s, frame_status, rgb, s->d_view, npx * 3);
}

// Runs at the first use: does tr_powf (tr_powf.h: glibc's algorithm with the tables the BUILD
// host's libm held) return what the powf of the C library this process RUNS with returns?  The
// library may be built on one machine and loaded on another; the specular closure's
// "bit for bit the host's powf" only holds when the two agree.
int powf_matches_this_host()
{
    static int cached = -1;
    if (cached >= 0) return cached;
    if (!tr::specular_is_exact()) return cached = 0;
    uint64_t x = 0x9E3779B97F4A7C15ull;
    int ok = 1;
    for (int i = 0; i < 20000 && ok; i++) {
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        // the closure's domain: base max(r.z, 0) in [0, 1], exponent 0..255 (util.rs:82)
        const float base = (i % 97 == 0) ? 0.0f : (i % 89 == 0) ? 1.0f : (float)((x >> 11) & 0xFFFFFFu) / 16777216.0f;
        const float e = (float)((x >> 40) & 0xFFu);
        const float a = tr::tr_powf(base, e), b = powf(base, e);
        if (memcmp(&a, &b, 4) != 0) ok = 0;
    }
    return cached = ok;
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
extern "C" {

int tr_abi_version(void) { return TR_ABI_VERSION; }

int tr_specular_exact(void) { return powf_matches_this_host(); }

const char *tr_last_error(void) { return tr::g_last_error.c_str(); }

int tr_selftest_device_math(int device, const float *x, const float *d, uint32_t n, uint32_t *out_u32,
                            int32_t *out_i32, uint32_t *out_u8, float *out_div, float *out_div_ref)
{
    if (!x || !d || !out_u32 || !out_i32 || !out_u8 || !out_div || !out_div_ref)
        return tr::fail(TR_E_INVALID, "null argument");
    if (device >= 0) HIP_TRY(hipSetDevice(device));
    void *buf[7] = {};
    int st = TR_OK;
    for (int i = 0; i < 7 && st == TR_OK; i++)
        if (hipMalloc(&buf[i], (size_t)(n ? n : 1) * 4) != hipSuccess) st = tr::fail(TR_E_HIP, "hipMalloc failed");
    if (st == TR_OK && (hipMemcpy(buf[0], x, (size_t)n * 4, hipMemcpyHostToDevice) != hipSuccess ||
                        hipMemcpy(buf[1], d, (size_t)n * 4, hipMemcpyHostToDevice) != hipSuccess))
        st = tr::fail(TR_E_HIP, "upload failed");
    if (st == TR_OK) {
        int rc = launch_selftest((const float *)buf[0], (const float *)buf[1], n, (uint32_t *)buf[2], (int32_t *)buf[3],
                                 (uint32_t *)buf[4], (float *)buf[5], (float *)buf[6], nullptr);
        if (rc || hipDeviceSynchronize() != hipSuccess) st = tr::fail(TR_E_HIP, "self-test kernel failed");
    }
    void *outs[5] = { out_u32, out_i32, out_u8, out_div, out_div_ref };
    for (int i = 0; i < 5 && st == TR_OK; i++)
        if (hipMemcpy(outs[i], buf[2 + i], (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess)
            st = tr::fail(TR_E_HIP, "download failed");
    for (int i = 0; i < 7; i++)
        if (buf[i]) (void)hipFree(buf[i]);
    return st;
}

int tr_selftest_shadow_fetch(int device, uint32_t width, uint32_t height, const float *plain, const float *stale,
                             const uint32_t *sclean, uint32_t n, const float *x, const float *y, uint32_t *out_plain,
                             uint32_t *out_flagged, uint32_t *err_plain, uint32_t *err_flagged)
{
    if (!plain || !stale || !sclean || !x || !y || !out_plain || !out_flagged || !err_plain || !err_flagged || width == 0 ||
        height == 0)
        return tr::fail(TR_E_INVALID, "null argument");
    if (device >= 0) HIP_TRY(hipSetDevice(device));
    const size_t npx = (size_t)width * height;
    const size_t n_tiles = (size_t)((width + TILE_W - 1) / TILE_W) * ((height + TILE_H - 1) / TILE_H);
    const size_t bytes[9] = { npx * 4, npx * 4, n_tiles * 4, (size_t)n * 4, (size_t)n * 4, (size_t)n * 4, (size_t)n * 4,
                              (size_t)n * 4, (size_t)n * 4 };
    const void *src[5] = { plain, stale, sclean, x, y };
    void *buf[9] = {};
    int st = TR_OK;
    for (int i = 0; i < 9 && st == TR_OK; i++)
        if (hipMalloc(&buf[i], bytes[i] ? bytes[i] : 4) != hipSuccess) st = tr::fail(TR_E_HIP, "hipMalloc failed");
    for (int i = 0; i < 5 && st == TR_OK; i++)
        if (hipMemcpy(buf[i], src[i], bytes[i], hipMemcpyHostToDevice) != hipSuccess) st = tr::fail(TR_E_HIP, "upload failed");
    if (st == TR_OK) {
        int rc = launch_selftest_shadow((const float *)buf[0], (const float *)buf[1], (const uint32_t *)buf[2], width, height,
                                        (const float *)buf[3], (const float *)buf[4], n, (uint32_t *)buf[5], (uint32_t *)buf[6],
                                        (uint32_t *)buf[7], (uint32_t *)buf[8], nullptr);
        if (rc || hipDeviceSynchronize() != hipSuccess) st = tr::fail(TR_E_HIP, "self-test kernel failed");
    }
    void *outs[4] = { out_plain, out_flagged, err_plain, err_flagged };
    for (int i = 0; i < 4 && st == TR_OK; i++)
        if (hipMemcpy(outs[i], buf[5 + i], (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess) st = tr::fail(TR_E_HIP, "download failed");
    for (int i = 0; i < 9; i++)
        if (buf[i]) (void)hipFree(buf[i]);
    return st;
}

int tr_selftest_device_unary(int device, int which, int exp_lo, int exp_hi, uint64_t *n_tested, uint64_t *n_bad,
                             uint32_t bad_bits[16])
{
    if (!n_tested || !n_bad || !bad_bits || which < 0 || which > 2 || exp_lo < -127 || exp_hi > 128 || exp_lo > exp_hi)
        return tr::fail(TR_E_INVALID, "bad argument");
    if (device >= 0) HIP_TRY(hipSetDevice(device));
    unsigned long long *d_n = nullptr;
    uint32_t *d_bits = nullptr;
    HIP_TRY(hipMalloc((void **)&d_n, 8));
    HIP_TRY(hipMalloc((void **)&d_bits, 64));
    HIP_TRY(hipMemset(d_n, 0, 8));
    HIP_TRY(hipMemset(d_bits, 0, 64));
    // every f32 with exponent in [exp_lo, exp_hi]: one contiguous range of bit patterns (positive
    // values; the reciprocal kernel checks -x beside x)
    const uint32_t first = (uint32_t)(exp_lo + 127) << 23;
    const uint64_t count = (uint64_t)(exp_hi - exp_lo + 1) << 23;
    int rc = launch_selftest_unary(which, first, count, d_n, d_bits, nullptr);
    int st = TR_OK;
    if (rc || hipDeviceSynchronize() != hipSuccess) st = tr::fail(TR_E_HIP, "self-test kernel failed");
    unsigned long long nb = 0;
    if (st == TR_OK && (hipMemcpy(&nb, d_n, 8, hipMemcpyDeviceToHost) != hipSuccess ||
                        hipMemcpy(bad_bits, d_bits, 64, hipMemcpyDeviceToHost) != hipSuccess))
        st = tr::fail(TR_E_HIP, "download failed");
    (void)hipFree(d_n);
    (void)hipFree(d_bits);
    *n_tested = count;
    *n_bad = nb;
    return st;
}

int tr_pipeline_count(void) { return P_COUNT; }

const char *tr_pipeline_name(int i) { return (i >= 0 && i < P_COUNT) ? kPipelines[i].name : nullptr; }

int tr_prepare_uniforms(int kind, tr_uniforms *u, uint32_t width, uint32_t height, const float light[3],
                        const float look_from[3], const float look_at[3], const float up[3])
{
    if (!u || !light || !look_from || !look_at || !up) return tr::fail(TR_E_INVALID, "null argument");
    return prepare_uniforms(kind, u, width, height, light, look_from, look_at, up);
}

int tr_scene_create(uint32_t width, uint32_t height, const tr_mesh *mesh, const tr_image_rgb8 tex[4],
                    const char *pipeline_name, const tr_options *opts, tr_scene **out)
{
    if (!out) return tr::fail(TR_E_INVALID, "null out pointer");
    *out = nullptr;
    tr_scene *s = new tr_scene();
    {
        std::lock_guard<std::mutex> lock(g_host_mutex);
        s->id = ++g_scene_serial;
    }
    int st = create(width, height, mesh, tex, pipeline_name, opts, s);
    if (st != TR_OK) {
        std::string keep = tr::g_last_error;
        destroy(s);
        tr::g_last_error = keep;
        return st;
    }
    *out = s;
    return TR_OK;
}

void tr_scene_destroy(tr_scene *s) { destroy(s); }

int tr_scene_clear(tr_scene *s)
{
    if (!s) return tr::fail(TR_E_INVALID, "null scene");
    s->z_fb_cleared = true;
    s->shadow_cleared = true;
    return TR_OK;
}

int tr_scene_set_light_direction(tr_scene *s, const float v[3])
{
    if (!s || !v) return tr::fail(TR_E_INVALID, "null argument");
    memcpy(s->view.light, v, sizeof s->view.light);
    return TR_OK;
}

int tr_scene_set_camera(tr_scene *s, const float look_from[3], const float look_at[3], const float up[3])
{
    if (!s || !look_from || !look_at || !up) return tr::fail(TR_E_INVALID, "null argument");
    memcpy(s->view.look_from, look_from, sizeof s->view.look_from);
    memcpy(s->view.look_at, look_at, sizeof s->view.look_at);
    memcpy(s->view.up, up, sizeof s->view.up);
    return TR_OK;
}

int tr_scene_render(tr_scene *s)
{
    if (!s) return tr::fail(TR_E_INVALID, "null scene");
    if (s->broken) return unusable();
    HIP_TRY(hipSetDevice(s->device));
    s->last.view = s->view;
    s->last.z_fb_cleared = s->z_fb_cleared;
    s->last.shadow_cleared = s->shadow_cleared;
    s->last.valid = true;
    s->last.inst = s->inst;
    s->last_was_group = false;
    if (!frame_is_groupable(s)) {
        // frames held back before it go first (it may render onto the last of them)
        int st = flush_deferred(s, false);
        if (st != TR_OK) return st;
        // a render without a clear depth-tests against the frame so far: its depth must be in memory
        if (!s->z_fb_cleared && (st = ensure_depth(s)) != TR_OK) return st;
        return render_frame(s);
    }
    // a cleared frame on the library's own stream: recorded now, rendered with its neighbours ("Automatic frame
    // groups").  Its constants are checked here, so that a camera the reference would panic on is this call's status.
    s->host_status = TR_OK;
    const PipelineDesc &pd = kPipelines[s->pipeline];
    for (int i = 0; i < pd.n_passes; i++) {
        DevUniforms du;
        int st = pass_uniforms(s, pd.pass[i], du);
        if (st != TR_OK) {
            s->host_status = st;
            return st;
        }
    }
    // (the frame's shadow pass is still to come, into the current slot: its matrix is known now)
    if (pd.n_passes == 2) note_shadow_matrix(s->slots[(size_t)s->cur_slot], s->uniforms.shadow_matrix);
    tr_scene::DeferredFrame f;
    f.p = s->view;
    f.fb = s->d_fb;
    f.inst = s->inst;
    s->deferred.push_back(f);
    s->z_fb_cleared = s->shadow_cleared = false;  // the frame has consumed the clear
    // (a loop that has filled sixteen groups in a row without anybody looking at a frame is a long run: its groups grow)
    const uint32_t target = s->auto_streak >= 16u ? long_run_group_size(s) : group_size(s);
    if (s->deferred.size() >= (size_t)target) {
        s->auto_streak++;
        return flush_deferred(s, true);
    }
    return TR_OK;
}

// The argument protocol of the tr_scene_render_frames family: frames_head, the call's own refusals, frames_tail, then
// render_frames.  The head: the arguments every form takes, and a scene that can still render.
static int frames_head(const tr_scene *s, uint32_t n_frames, const tr_frame_params *frames)
{
    if (!s || (n_frames && !frames)) return tr::fail(TR_E_INVALID, "null argument");
    return s->broken ? unusable() : TR_OK;
}

// The tail: no frames are TR_OK without a look at the list or the device (`none`: the call is over); else every colour
// target of the list must be one, and the scene's device becomes the current one.
static int frames_tail(const tr_scene *s, uint32_t n_frames, void *const *frame_buffers_device, bool &none)
{
    none = n_frames == 0;
    if (none) return TR_OK;
    if (frame_buffers_device)
        for (uint32_t i = 0; i < n_frames; i++)
            if (!frame_buffers_device[i]) return tr::fail(TR_E_INVALID, "null frame buffer in the list");
    HIP_TRY(hipSetDevice(s->device));
    return TR_OK;
}

int tr_scene_render_frames(tr_scene *s, uint32_t n_frames, const tr_frame_params *frames, void *const *frame_buffers_device)
{
    bool none = false;
    int st = frames_head(s, n_frames, frames);
    if (st != TR_OK || (st = frames_tail(s, n_frames, frame_buffers_device, none)) != TR_OK || none) return st;
    return render_frames(s, n_frames, frames, nullptr, frame_buffers_device);
}

// tr_scene_set_instances / tr_scene_set_instance_transforms: `table` holds n entries of `stride` floats.
static int set_table(tr_scene *s, uint32_t n, uint32_t stride, const float *table)
{
    if (!s) return tr::fail(TR_E_INVALID, "null scene");
    int st = check_instances(s, n, table);
    if (st != TR_OK) return st;
    HIP_TRY(hipSetDevice(s->device));
    if ((st = grow_for_instances(s, n)) != TR_OK) return st;
    tr_scene::InstRef r;
    if (n && (st = upload_instances(s, n, stride, table, r)) != TR_OK) return st;
    r.pose = s->inst.pose;  // (the table places the mesh under the current pose)
    use_inst(s, r);
    return TR_OK;
}

// tr_scene_render_frames_instanced / tr_scene_render_frames_transformed: frame i draws entries [i n, (i + 1) n) of `tables`.
static int render_frames_tables(tr_scene *s, uint32_t n_frames, const tr_frame_params *frames, uint32_t n, uint32_t stride,
                                const float *tables, void *const *frame_buffers_device)
{
    bool none = false;
    int st = frames_head(s, n_frames, frames);
    if (st != TR_OK || (st = check_instances(s, n, tables)) != TR_OK) return st;
    // (no frames: no entries, so this never comes before the tail's TR_OK)
    if ((uint64_t)n_frames * n > 0xFFFFFFFFull) return tr::fail(TR_E_INVALID, "instance tables too large");
    if ((st = frames_tail(s, n_frames, frame_buffers_device, none)) != TR_OK || none) return st;
    if ((st = grow_for_instances(s, n)) != TR_OK) return st;
    // all the frames' tables as one block: frame i draws entries [i n, (i + 1) n)
    std::vector<tr_scene::InstRef> insts(n_frames);
    if (n) {
        tr_scene::InstRef all;
        if ((st = upload_instances(s, n_frames * n, stride, tables, all)) != TR_OK) return st;
        for (uint32_t i = 0; i < n_frames; i++) {
            insts[i] = all;
            insts[i].off = i * n;
            insts[i].n = n;
        }
    }
    for (uint32_t i = 0; i < n_frames; i++) insts[i].pose = s->inst.pose;  // every frame draws the current pose
    return render_frames(s, n_frames, frames, insts.data(), frame_buffers_device);
}

int tr_scene_set_instances(tr_scene *s, uint32_t n_instances, const tr_instance *instances)
{
    static_assert(sizeof(tr_instance) == sizeof(float) * tr::INST_FLOATS, "tr_instance is four floats");
    return set_table(s, n_instances, tr::INST_FLOATS, reinterpret_cast<const float *>(instances));
}

int tr_scene_set_instance_transforms(tr_scene *s, uint32_t n_instances, const tr_instance_xform *table)
{
    static_assert(sizeof(tr_instance_xform) == sizeof(float) * tr::INST_XFORM_FLOATS, "tr_instance_xform is 24 floats");
    return set_table(s, n_instances, tr::INST_XFORM_FLOATS, reinterpret_cast<const float *>(table));
}

int tr_scene_render_frames_instanced(tr_scene *s, uint32_t n_frames, const tr_frame_params *frames, uint32_t n_instances,
                                     const tr_instance *instances, void *const *frame_buffers_device)
{
    return render_frames_tables(s, n_frames, frames, n_instances, tr::INST_FLOATS, reinterpret_cast<const float *>(instances),
                                frame_buffers_device);
}

int tr_scene_render_frames_transformed(tr_scene *s, uint32_t n_frames, const tr_frame_params *frames, uint32_t n_instances,
                                       const tr_instance_xform *table, void *const *frame_buffers_device)
{
    return render_frames_tables(s, n_frames, frames, n_instances, tr::INST_XFORM_FLOATS, reinterpret_cast<const float *>(table),
                                frame_buffers_device);
}

int tr_scene_set_morph_targets(tr_scene *s, uint32_t n_targets, const float *dpos, const float *dnrm)
{
    if (!s) return tr::fail(TR_E_INVALID, "null scene");
    if (n_targets > (uint32_t)TR_MORPH_MAX_TARGETS) return tr::fail(TR_E_INVALID, "more than TR_MORPH_MAX_TARGETS morph targets");
    if (n_targets && ((s->n_pos && !dpos) || (s->n_nrm && !dnrm))) return tr::fail(TR_E_INVALID, "null delta array");
    HIP_TRY(hipSetDevice(s->device));
    // the deltas gathered per polygon like the mesh's rows (uv floats: zero, never read as deltas)
    std::vector<float> rows((size_t)n_targets * s->n_rows * TRI_FLOATS, 0.0f);
    const std::vector<float> no_tex(3, 0.0f);
    for (uint32_t k = 0; k < n_targets; k++)
        for (uint32_t t = 0; t < s->n_rows; t++) {
            uint32_t ix[9];
            memcpy(ix, &s->mesh_idx[9u * (size_t)t], sizeof ix);
            ix[1] = ix[4] = ix[7] = 0u;
            gather_polygon(dpos + (size_t)k * s->n_pos * 3u, no_tex.data(), dnrm + (size_t)k * s->n_nrm * 3u, ix,
                           &rows[((size_t)k * s->n_rows + t) * TRI_FLOATS]);
        }
    // (frames issued so far keep their poses: their rows are blended before the deltas change)
    int st = swap_device_array(s, s->d_delta, n_targets != 0u, rows.data(), rows.size());
    if (st != TR_OK) return st;
    s->n_targets = n_targets;
    trim_pose_pool(s, 0);  // (everything queued has run: the free rows go back to the device)
    // no weights of the old targets stay current (frames already rendered keep their rows); the palette does: the skin
    // does not depend on the targets
    tr_scene::InstRef r = s->inst;
    r.pose = make_pose(s, nullptr, pose_palette(s, s->inst.pose));
    use_inst(s, r);
    return TR_OK;
}

int tr_scene_set_morph_weights(tr_scene *s, uint32_t n_weights, const float *w)
{
    if (!s) return tr::fail(TR_E_INVALID, "null scene");
    int st = check_weight_count(s, n_weights);
    if (st != TR_OK) return st;
    if (n_weights && !w) return tr::fail(TR_E_INVALID, "null weights");
    tr_scene::InstRef r = s->inst;
    r.pose = make_pose(s, n_weights ? w : nullptr, pose_palette(s, s->inst.pose));  // (the palette stays)
    use_inst(s, r);
    return TR_OK;
}

int tr_scene_render_frames_morphed(tr_scene *s, uint32_t n_frames, const tr_frame_params *frames, uint32_t n_weights,
                                   const float *weights, void *const *frame_buffers_device)
{
    bool none = false;
    int st = frames_head(s, n_frames, frames);
    if (st != TR_OK || (st = check_weight_count(s, n_weights)) != TR_OK) return st;
    if (n_weights && n_frames && !weights) return tr::fail(TR_E_INVALID, "null weights");
    if ((st = frames_tail(s, n_frames, frame_buffers_device, none)) != TR_OK || none) return st;
    // the current table under a pose per frame
    return render_frames(s, n_frames, frames, nullptr, frame_buffers_device, POSED_WEIGHTS, n_weights ? weights : nullptr);
}

int tr_scene_debug_morph_rows(tr_scene *s)
{
    if (!s) return tr::fail(TR_E_INVALID, "null scene");
    return (int)s->pose_rows_live;
}

// The rule of tr_morph.h over the indexed arrays, on the host.  Needs no GPU.
int tr_morph_mesh(const tr_mesh *mesh, uint32_t n_targets, const float *dpos, const float *dnrm, const float *w, float *pos_out,
                  float *nrm_out)
{
    if (!mesh || (n_targets && !w)) return tr::fail(TR_E_INVALID, "null argument");
    if (n_targets > (uint32_t)TR_MORPH_MAX_TARGETS) return tr::fail(TR_E_INVALID, "more than TR_MORPH_MAX_TARGETS morph targets");
    if ((mesh->n_pos && (!mesh->pos || !pos_out || (n_targets && !dpos))) || (mesh->n_nrm && (!mesh->nrm || !nrm_out || (n_targets && !dnrm))))
        return tr::fail(TR_E_INVALID, "null array");
    const size_t np = (size_t)mesh->n_pos * 3u, nn = (size_t)mesh->n_nrm * 3u;
    for (size_t i = 0; i < np; i++) pos_out[i] = tr::morph_component(mesh->pos[i], n_targets, w, dpos + i, np);
    for (size_t i = 0; i < nn; i++) nrm_out[i] = tr::morph_component(mesh->nrm[i], n_targets, w, dnrm + i, nn);
    return TR_OK;
}

int tr_scene_set_skin(tr_scene *s, uint32_t n_bones, const uint32_t *bone, const float *weight)
{
    if (!s) return tr::fail(TR_E_INVALID, "null scene");
    if (n_bones > (uint32_t)TR_SKIN_MAX_BONES) return tr::fail(TR_E_INVALID, "more than TR_SKIN_MAX_BONES bones");
    if (n_bones && s->n_pos && (!bone || !weight)) return tr::fail(TR_E_INVALID, "null influence array");
    for (size_t i = 0; n_bones && i < (size_t)s->n_pos * tr::SKIN_INFLUENCES; i++)
        if (bone[i] >= n_bones) return tr::fail(TR_E_INVALID, "bone index beyond n_bones");
    HIP_TRY(hipSetDevice(s->device));
    // the influences gathered per polygon like the mesh's rows
    std::vector<uint32_t> rows(n_bones ? (size_t)s->n_rows * tr::SKIN_ROW_WORDS : 0u);
    if (n_bones) tr::gather_skin_rows(s->mesh_idx.data(), s->n_rows, bone, weight, rows.data());
    // (frames issued so far keep their palettes: their rows are skinned before the skin changes)
    int st = swap_device_array(s, s->d_skin, n_bones != 0u, rows.data(), rows.size());
    if (st != TR_OK) return st;
    s->n_bones = n_bones;
    trim_pose_pool(s, 0);  // (everything queued has run: the free rows go back to the device)
    // no palette of the old skin stays current (frames already rendered keep their rows); the morph weights do
    tr_scene::InstRef r = s->inst;
    r.pose = make_pose(s, pose_weights(s, s->inst.pose), nullptr);
    use_inst(s, r);
    return TR_OK;
}

int tr_scene_set_bone_palette(tr_scene *s, uint32_t n_bones, const tr_instance_xform *palette)
{
    if (!s) return tr::fail(TR_E_INVALID, "null scene");
    int st = check_bone_count(s, n_bones);
    if (st != TR_OK) return st;
    if (n_bones && !palette) return tr::fail(TR_E_INVALID, "null palette");
    tr_scene::InstRef r = s->inst;
    r.pose = make_pose(s, pose_weights(s, s->inst.pose), n_bones ? reinterpret_cast<const float *>(palette) : nullptr);  // (the weights stay)
    use_inst(s, r);
    return TR_OK;
}

int tr_scene_render_frames_skinned(tr_scene *s, uint32_t n_frames, const tr_frame_params *frames, uint32_t n_bones,
                                   const tr_instance_xform *palettes, void *const *frame_buffers_device)
{
    bool none = false;
    int st = frames_head(s, n_frames, frames);
    if (st != TR_OK || (st = check_bone_count(s, n_bones)) != TR_OK) return st;
    if (n_bones && n_frames && !palettes) return tr::fail(TR_E_INVALID, "null palettes");
    if ((st = frames_tail(s, n_frames, frame_buffers_device, none)) != TR_OK || none) return st;
    // the current table and morph weights under a palette per frame
    return render_frames(s, n_frames, frames, nullptr, frame_buffers_device, POSED_PALETTES,
                         n_bones ? reinterpret_cast<const float *>(palettes) : nullptr);
}

// The rule of tr_skin.h over the indexed arrays, on the host: the unrolled skinned mesh.  Needs no GPU.
int tr_skin_mesh(const tr_mesh *mesh, uint32_t n_bones, const uint32_t *bone, const float *weight, const tr_instance_xform *palette,
                 float *pos_out, float *nrm_out, uint32_t *idx_out)
{
    if (!mesh) return tr::fail(TR_E_INVALID, "null argument");
    if (n_bones == 0 || n_bones > (uint32_t)TR_SKIN_MAX_BONES) return tr::fail(TR_E_INVALID, "n_bones must be 1 .. TR_SKIN_MAX_BONES");
    if (!palette || (mesh->n_pos && (!bone || !weight))) return tr::fail(TR_E_INVALID, "null argument");
    if (mesh->n_tri && (!mesh->pos || !mesh->nrm || !mesh->idx || !pos_out || !nrm_out || !idx_out)) return tr::fail(TR_E_INVALID, "null array");
    for (size_t i = 0; i < (size_t)mesh->n_pos * tr::SKIN_INFLUENCES; i++)
        if (bone[i] >= n_bones) return tr::fail(TR_E_INVALID, "bone index beyond n_bones");
    for (size_t i = 0; i < (size_t)mesh->n_tri * 9u; i += 3u)
        if (mesh->idx[i] >= mesh->n_pos || mesh->idx[i + 2u] >= mesh->n_nrm) return tr::fail(TR_E_INVALID, "mesh index out of range");
    tr::skin_mesh_unrolled(mesh->pos, mesh->nrm, mesh->idx, mesh->n_tri, bone, weight, reinterpret_cast<const float *>(palette), pos_out,
                           nrm_out, idx_out);
    return TR_OK;
}

// The concatenated mesh a transform table draws, on the host: the vertex stage's own xform_position / xform_normal
// (tr_shaders.h) over the indexed arrays.  Needs no GPU.
int tr_instance_transform_mesh(const tr_mesh *mesh, uint32_t n_instances, const tr_instance_xform *table, float *pos_out,
                               float *nrm_out)
{
    if (!mesh || (n_instances && !table)) return tr::fail(TR_E_INVALID, "null argument");
    if ((mesh->n_pos && (!mesh->pos || !pos_out)) || (mesh->n_nrm && (!mesh->nrm || !nrm_out)))
        return tr::fail(TR_E_INVALID, "null array");
    for (uint32_t k = 0; k < n_instances; k++) {
        const tr_instance_xform &e = table[k];
        float *po = pos_out + (size_t)k * mesh->n_pos * 3u, *no = nrm_out + (size_t)k * mesh->n_nrm * 3u;
        for (uint32_t i = 0; i < mesh->n_pos; i++) {
            float x = mesh->pos[3u * i], y = mesh->pos[3u * i + 1u], z = mesh->pos[3u * i + 2u];
            tr::xform_position(e.m, x, y, z);
            po[3u * i] = x;
            po[3u * i + 1u] = y;
            po[3u * i + 2u] = z;
        }
        for (uint32_t i = 0; i < mesh->n_nrm; i++) {
            float a = mesh->nrm[3u * i], b = mesh->nrm[3u * i + 1u], c = mesh->nrm[3u * i + 2u];
            tr::xform_normal(e.n, a, b, c);
            no[3u * i] = a;
            no[3u * i + 1u] = b;
            no[3u * i + 2u] = c;
        }
    }
    return TR_OK;
}

int tr_scene_interior_tiles(tr_scene *s)
{
    if (!s) return tr::fail(TR_E_INVALID, "null scene");
    return s->fused_interior > 0 ? 1 : 0;
}

int tr_scene_frames_per_launch(tr_scene *s) { return s ? (int)group_size(s) : tr::fail(TR_E_INVALID, "null scene"); }

int tr_scene_frames_kept(tr_scene *s)
{
    if (!s) return tr::fail(TR_E_INVALID, "null scene");
    return s->last_was_group ? (int)s->tail.params.size() : 0;
}

int tr_scene_select_frame(tr_scene *s, uint32_t back)
{
    if (!s) return tr::fail(TR_E_INVALID, "null scene");
    if (!s->last_was_group || back >= s->tail.params.size())
        return tr::fail(TR_E_INVALID, "tr_scene_select_frame: no such frame (tr_scene_frames_kept tells how many the last tr_scene_render_frames left)");
    HIP_TRY(hipSetDevice(s->device));
    const size_t k = s->tail.params.size() - 1u - back;
    s->view = s->tail.params[k];   // (for good: the selection is the scene's state from here on)
    use_inst(s, s->tail.inst[k]);
    return use_slot(s, s->tail.slot[k], s->tail.fbs.empty() ? nullptr : (uint8_t *)s->tail.fbs[k]);
}

int tr_scene_set_auto_group(tr_scene *s, int on)
{
    if (!s) return tr::fail(TR_E_INVALID, "null scene");
    HIP_TRY(hipSetDevice(s->device));
    int st = submit_pending(s);  // frames held back so far are rendered as they were issued
    s->auto_group = on != 0;
    return st;
}

int tr_scene_flush(tr_scene *s)
{
    if (!s) return tr::fail(TR_E_INVALID, "null scene");
    HIP_TRY(hipSetDevice(s->device));
    return submit_pending(s);
}

int tr_scene_sync(tr_scene *s)
{
    if (!s) return tr::fail(TR_E_INVALID, "null scene");
    return sync_and_status(s);
}

void *tr_scene_frame_buffer_device(tr_scene *s) { return s ? s->d_fb : nullptr; }

int tr_scene_set_frame_buffer_device(tr_scene *s, void *frame_buffer_device)
{
    if (!s) return tr::fail(TR_E_INVALID, "null scene");
    HIP_TRY(hipSetDevice(s->device));
    return use_slot(s, s->cur_slot, (uint8_t *)frame_buffer_device, true);
}

int tr_band_rows(uint32_t height, uint32_t n_ranks, uint32_t rank, uint32_t *row0, uint32_t *row1)
{
    if (!row0 || !row1 || n_ranks == 0 || rank >= n_ranks || height < n_ranks)
        return tr::fail(TR_E_INVALID, "tr_band_rows: need rank < n_ranks <= height");
    *row0 = (uint32_t)(((uint64_t)rank * height) / n_ranks);
    *row1 = (uint32_t)(((uint64_t)(rank + 1u) * height) / n_ranks);
    return TR_OK;
}

int tr_scene_set_stream(tr_scene *s, void *hip_stream)
{
    if (!s) return tr::fail(TR_E_INVALID, "null scene");
    HIP_TRY(hipSetDevice(s->device));
    {
        int sp = submit_pending(s);
        if (sp != TR_OK) return sp;
    }
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (s->own_stream) (void)hipStreamDestroy(s->stream);
    s->own_stream = false;
    if (hip_stream) {
        s->stream = (hipStream_t)hip_stream;
    } else {
        HIP_TRY(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
        s->own_stream = true;
    }
    return TR_OK;
}

int tr_scene_get_frame_buffer(tr_scene *s, uint8_t *rgb)
{
    if (!s || !rgb) return tr::fail(TR_E_INVALID, "null argument");
    int fst = sync_and_status(s);
    if (fatal(fst)) return fst;
    int st = flush_clear_color(s);
    if (st != TR_OK) return st;
    return finish_read_back(s, fst, rgb, s->d_fb, (size_t)s->width * s->height * 3);
}

int tr_scene_get_frame_buffer_async(tr_scene *s, uint8_t *rgb)
{
    if (!s || !rgb) return tr::fail(TR_E_INVALID, "null argument");
    HIP_TRY(hipSetDevice(s->device));
    int st = flush_clear_color(s);
    if (st != TR_OK) return st;
    st = submit_pending(s);
    if (st != TR_OK) return st;
    const size_t bytes = (size_t)s->width * s->height * 3;
    // same stream as the tile kernels: after the frame, before the next one overwrites it.  Into memory from
    // tr_host_alloc only the tiles that are not zeros on both sides travel (k_read_back); any other buffer gets
    // the whole frame from the copy engine.
    // The sparse form needs a scene that renders the WHOLE frame: k_read_back writes the tiles of the scene's band only,
    // and "the buffer ends up holding the complete frame" must hold for a band scene too (whose other rows, in a
    // caller's all-gather buffer, come from other ranks): such a scene takes the copy engine.
    void *mapped = nullptr;
    uint64_t serial = 0, gen = 0;
    bool mine = false;  // this scene was the buffer's last writer
    {
        std::lock_guard<std::mutex> lock(g_host_mutex);
        auto it = g_host_allocs.find(rgb);
        if (it != g_host_allocs.end()) {
            if (it->second.bytes >= bytes && whole_frame(s) && s->width % 16u == 0u && s->d_fbclean) {
                mapped = it->second.device;
                serial = it->second.serial;
                mine = it->second.writer == s->id;
                gen = it->second.gen;
            }
            // (whichever way the frame travels: from now on this scene is the last writer, and every other scene's
            // record of the buffer has lapsed)
            it->second.writer = s->id;
            it->second.gen += 1u;
            if (mapped) gen = it->second.gen - 1u;
        }
    }
    if (mapped) {
        uint32_t *host_clean = nullptr;
        for (tr_scene::HostFlags &f : s->host_flags)
            if (f.host == rgb) {
                // the address of a buffer that has been freed (another buffer now), or somebody else -- another scene's
                // read-back, the caller (tr_scene_host_buffer_written) -- has written the buffer since: content unknown
                if (f.serial != serial || !mine || f.gen != gen) {
                    HIP_TRY(hipMemsetAsync(f.clean, 0, (size_t)s->n_tiles * 4, s->stream));
                    f.serial = serial;
                }
                f.gen = gen + 1u;
                host_clean = f.clean;
            }
        if (!host_clean) {
            if (s->host_flags.size() >= 64u) {  // (a caller that cycles through many buffers: forget the oldest)
                HIP_TRY(hipStreamSynchronize(s->stream));
                dev_free(s->host_flags.front().clean);
                s->host_flags.erase(s->host_flags.begin());
            }
            if ((st = dev_alloc(&host_clean, (size_t)s->n_tiles))) return st;
            HIP_TRY(hipMemsetAsync(host_clean, 0, (size_t)s->n_tiles * 4, s->stream));  // content of the buffer unknown
            s->host_flags.push_back({ rgb, serial, host_clean, gen + 1u });
        }
        int rc = launch_read_back(s->d_fb, (uint8_t *)mapped, s->d_fbclean, host_clean, s->frame, s->stream);
        if (rc) return launch_status(rc, "k_read_back");
    } else {
        HIP_TRY(hipMemcpyAsync(rgb, s->d_fb, bytes, hipMemcpyDeviceToHost, s->stream));
    }
    s->quiescent = false;
    handed_on(s);
    return TR_OK;
}

int tr_scene_resolve(tr_scene *s, uint32_t factor, void *out)
{
    if (!s || !out) return tr::fail(TR_E_INVALID, "null argument");
    int st = check_resolve(s, factor);
    if (st != TR_OK) return st;
    HIP_TRY(hipSetDevice(s->device));
    void *target = nullptr;
    st = classify_out(out, resolved_bytes(s, factor), "tr_scene_resolve", "tr_scene_get_resolved", "resolved frame", &target);
    if (st == TR_OK) st = enqueue_resolve(s, factor, (uint8_t *)target);
    if (st == TR_OK) handed_on(s);
    return st;
}

int tr_scene_get_resolved(tr_scene *s, uint32_t factor, uint8_t *rgb)
{
    if (!s || !rgb) return tr::fail(TR_E_INVALID, "null argument");
    int st = check_resolve(s, factor);
    if (st != TR_OK) return st;
    return get_stage(s, rgb, resolved_bytes(s, factor), nullptr, [&](uint8_t *o) { return enqueue_resolve(s, factor, o); });
}

int tr_scene_composite(tr_scene *dst, tr_scene *src, uint32_t winner_base)
{
    if (!dst || !src) return tr::fail(TR_E_INVALID, "tr_scene_composite: null scene");
    if (dst == src) return tr::fail(TR_E_INVALID, "tr_scene_composite: dst and src are the same scene");
    if (dst->device != src->device) return tr::fail(TR_E_INVALID, "tr_scene_composite: the scenes are on different devices");
    if (dst->width != src->width || dst->height != src->height)
        return tr::fail(TR_E_INVALID, "tr_scene_composite: the scenes' frames differ in width or height");
    if (dst->frame.band_y0 != src->frame.band_y0 || dst->frame.band_y1 != src->frame.band_y1)
        return tr::fail(TR_E_INVALID, "tr_scene_composite: the scenes render different bands (tr_options.band_row0/1)");
    if (dst->d_winner && !src->d_winner)
        return tr::fail(TR_E_INVALID, "tr_scene_composite: dst has TR_OPT_WINNER_TAP and src has not");
    if (dst->broken || src->broken) return unusable();
    HIP_TRY(hipSetDevice(dst->device));
    if (src->z_fb_cleared) return TR_OK;  // a logically cleared frame covers no pixel
    int st = depth_in_memory(src);
    // dst: its frame on its way and its depth in memory too, and a pending clear made real (its z: every flag up)
    if (st == TR_OK) st = submit_pending(dst);
    if (st == TR_OK && !dst->z_fb_cleared) st = ensure_depth(dst);
    if (st == TR_OK) st = flush_clear_color(dst);
    if (st == TR_OK) st = need_z(dst, dst->cur_slot);
    if (st != TR_OK) return st;
    CompositeArgs a = {};
    a.dst_z = dst->d_z;
    a.dst_fb = dst->d_fb;
    a.dst_winner = dst->d_winner;
    a.dst_zclean = dst->d_zclean;
    a.dst_fbclean = dst->d_fbclean;
    a.src_z = src->d_z;
    a.src_fb = src->d_fb;
    a.src_winner = src->d_winner;
    // (src's colour-clean flags say less than its z flags -- a set belongs to one colour buffer and is forgotten when a
    // caller's buffer is handed over again or the winner tap was last written with another target's frame
    // (select_fb_flags), while the z flags always describe the slot's depth: the skip goes by the z flags alone)
    a.src_zclean = src->d_zclean;
    a.frame = dst->frame;
    a.winner_base = winner_base;
    st = cross_scene_launch(dst, src, [&] {
        Timed t(dst, K_COMPOSITE);
        int rc = launch_composite(a, dst->stream);
        return rc ? launch_status(rc, "k_composite") : TR_OK;
    });
    if (st == TR_OK) dst->slots[(size_t)dst->cur_slot].z_deferred = false;  // (the merged depth is in memory)
    return st;
}

// The rule of tr_composite.h over caller's arrays, on the host.  Needs no GPU.
int tr_composite_host(size_t n_pixels, float *z_dst, uint8_t *rgb_dst, uint32_t *win_dst, const float *z_src, const uint8_t *rgb_src,
                      const uint32_t *win_src, uint32_t winner_base)
{
    if (n_pixels && (!z_dst || !rgb_dst || !z_src || !rgb_src)) return tr::fail(TR_E_INVALID, "tr_composite_host: null argument");
    if (n_pixels && win_dst && !win_src) return tr::fail(TR_E_INVALID, "tr_composite_host: win_dst without win_src");
    for (size_t i = 0; i < n_pixels; i++) {
        if (!composite_wins(z_src[i], z_dst[i])) continue;
        z_dst[i] = z_src[i];
        memcpy(rgb_dst + 3 * i, rgb_src + 3 * i, 3);
        if (win_dst) win_dst[i] = composite_winner(win_src[i], winner_base);
    }
    return TR_OK;
}

namespace {

// tr_scene_render_shadow_pass / tr_scene_render_colour_pass: one pass of a two-pass pipeline, through run_pass like a
// frame of tr_scene_render's -- but submitted at once, never fused, and handed on: recover_from_overflow would replay
// s->last, the scene's own shadow pass included, over a buffer that may since have been merged.
int render_split_pass(tr_scene *s, bool colour, const char *who)
{
    if (!s) return tr::fail(TR_E_INVALID, std::string(who) + ": null scene");
    const PipelineDesc &pd = kPipelines[s->pipeline];
    if (pd.n_passes != 2)
        return tr::fail(TR_E_INVALID, std::string(who) + ": the scene's pipeline `" + pd.name + "` has one pass (shadow and occlusion have two)");
    if (s->broken) return unusable();
    HIP_TRY(hipSetDevice(s->device));
    int st = submit_pending(s);  // what tr_scene_render holds back goes first
    if (st != TR_OK) return st;
    s->host_status = TR_OK;
    if (colour) {
        // without a clear the pass depth-tests against the frame so far: its depth must be in memory
        if (!s->z_fb_cleared && (st = ensure_depth(s)) != TR_OK) return st;
        // the buffer as it stands is looked up under the matrix it was rendered (or merged) under; the reference's
        // second prepare leaves the first one's shadow matrix in place the same way (shader.rs:259-279)
        const tr_scene::FrameSlot &slot = s->slots[(size_t)s->cur_slot];
        if (slot.shadow_matrix_set) memcpy(s->uniforms.shadow_matrix, slot.shadow_matrix, sizeof slot.shadow_matrix);
    }
    st = run_pass(s, pd.pass[colour ? 1 : 0]);
    if (st == TR_OK) st = submit_pending_tiles(s);
    if (st != TR_OK) {
        s->host_status = st;
        return st;
    }
    handed_on(s);
    return TR_OK;
}

}  // namespace

int tr_scene_render_shadow_pass(tr_scene *s) { return render_split_pass(s, false, "tr_scene_render_shadow_pass"); }

int tr_scene_render_colour_pass(tr_scene *s) { return render_split_pass(s, true, "tr_scene_render_colour_pass"); }

int tr_scene_shadow_merge(tr_scene *dst, tr_scene *src)
{
    if (!dst || !src) return tr::fail(TR_E_INVALID, "tr_scene_shadow_merge: null scene");
    if (dst == src) return tr::fail(TR_E_INVALID, "tr_scene_shadow_merge: dst and src are the same scene");
    if (dst->device != src->device) return tr::fail(TR_E_INVALID, "tr_scene_shadow_merge: the scenes are on different devices");
    if (dst->width != src->width || dst->height != src->height)
        return tr::fail(TR_E_INVALID, "tr_scene_shadow_merge: the scenes' frames differ in width or height");
    if (kPipelines[dst->pipeline].n_passes != 2 || kPipelines[src->pipeline].n_passes != 2)
        return tr::fail(TR_E_INVALID, "tr_scene_shadow_merge: a scene's pipeline has one pass and no shadow buffer of its own "
                                      "(shadow and occlusion have two)");
    if (dst->broken || src->broken) return unusable();
    if (src->shadow_cleared) return TR_OK;  // a logically cleared buffer holds f32::MIN alone: it replaces nothing
    tr_scene::FrameSlot &ds = dst->slots[(size_t)dst->cur_slot];
    const tr_scene::FrameSlot &ss = src->slots[(size_t)src->cur_slot];
    // (a buffer no shadow pass has filled since the scene was created has no matrix: it holds the zeros of Buffer::new,
    // shader.rs:46-47, which merge by the rule under any)
    if (!dst->shadow_cleared && ds.shadow_matrix_set && ss.shadow_matrix_set &&
        memcmp(ds.shadow_matrix, ss.shadow_matrix, sizeof ds.shadow_matrix) != 0)
        return tr::fail(TR_E_INVALID, "tr_scene_shadow_merge: the shadow buffers were rendered under different shadow matrices "
                                      "(light, look_at, up or frame size differ)");
    HIP_TRY(hipSetDevice(dst->device));
    // both buffers on their way; a pending clear of dst made real (every flag up)
    int st = submit_pending(src);
    if (st == TR_OK) st = submit_pending(dst);
    if (st == TR_OK) st = flush_clear_shadow(dst);
    if (st != TR_OK) return st;
    ShadowMergeArgs a = {};
    a.dst = dst->d_shadow;
    a.dst_clean = dst->d_sclean;
    a.src = src->d_shadow;
    a.src_clean = src->d_sclean;
    a.frame = dst->frame_full;
    // (handed on: replaying a frame after a bin overflow would run the scene's own shadow pass over the merged buffer)
    st = cross_scene_launch(dst, src, [&] {
        Timed t(dst, K_SHADOW_MERGE);
        int rc = launch_shadow_merge(a, dst->stream);
        return rc ? launch_status(rc, "k_shadow_merge") : TR_OK;
    });
    if (st == TR_OK && ss.shadow_matrix_set) note_shadow_matrix(ds, ss.shadow_matrix);  // (equal already, or dst's buffer had none)
    return st;
}

// The rule of tr_shadow_merge.h over caller's arrays, on the host.  Needs no GPU.
int tr_shadow_merge_host(size_t n, float *dst, const float *src)
{
    if (n && (!dst || !src)) return tr::fail(TR_E_INVALID, "tr_shadow_merge_host: null argument");
    for (size_t i = 0; i < n; i++) dst[i] = shadow_merge(src[i], dst[i]);
    return TR_OK;
}

// ---------------------------------------------------------------------------------------------
// Dynamic textures
// ---------------------------------------------------------------------------------------------
namespace {

// Does [p, p + bytes) meet one of the scene's own texel arrays?
bool overlaps_texels(const tr_scene *s, const void *p, size_t bytes)
{
    auto meets = [&](const void *q, size_t n) {
        return q && (const uint8_t *)p < (const uint8_t *)q + n && (const uint8_t *)q < (const uint8_t *)p + bytes;
    };
    bool hit = meets(s->d_packed, s->packed_count * 4u);
    for (int k = 0; k < 4; k++) hit = hit || meets(s->d_texel[k], (size_t)s->tex.w[k] * s->tex.h[k] * 4u);
    return hit;
}

// Enqueues the repack of image `which` from `src_device` (w x h rgb8 rows; src_clean / all_clean: the colour-clean flags
// of the frame it is, PackArgs) on s's stream: behind everything s has been asked to render -- frames held back are
// submitted first and keep the old texture, every tile kernel issued so far is on the stream -- and behind `producer`'s
// work (an event on its stream; its stream then waits for the kernel, as in tr_scene_composite).  The setup streams
// wait for it as well: a later chain's k_lit reads the set.  *done (may be null) is recorded behind the kernel.
int enqueue_pack(tr_scene *s, uint32_t which, const uint8_t *src_device, const uint32_t *src_clean, bool all_clean, tr_scene *producer,
                 hipEvent_t done)
{
    int st = submit_pending(s);
    if (st == TR_OK && producer && producer != s) st = submit_pending(producer);
    if (st != TR_OK) return st;
    if (!s->ev_tex) HIP_TRY(hipEventCreateWithFlags(&s->ev_tex, hipEventDisableTiming));
    const bool other_scene = producer && producer != s;
    if (other_scene) {
        if (!producer->ev_comp_ready) HIP_TRY(hipEventCreateWithFlags(&producer->ev_comp_ready, hipEventDisableTiming));
        if (!s->ev_comp_done) HIP_TRY(hipEventCreateWithFlags(&s->ev_comp_done, hipEventDisableTiming));
    }
    PackArgs a = {};
    a.src = src_device;
    a.src_clean = src_clean;
    a.src_all_clean = all_clean ? 1u : 0u;
    a.texel = s->d_texel[which];
    a.set = s->d_packed;
    a.w = s->tex.w[which];
    a.h = s->tex.h[which];
    a.bpr = s->tex.packed_bpr;
    a.fs = s->set_fs;
    a.mode = s->d_packed ? pack_mode(s->set_fs, which) : 0u;
    // word 0 of a four-word set is rebuilt from the new texel and the other image's plain array
    if (a.mode == PACK_COLOUR && s->set_fs == FS_SPECULAR) a.other = s->d_texel[3];
    if (a.mode == PACK_SPEC) a.other = s->d_texel[0];
    if (other_scene) {
        HIP_TRY(hipEventRecord(producer->ev_comp_ready, producer->stream));
        HIP_TRY(hipStreamWaitEvent(s->stream, producer->ev_comp_ready, 0));
    }
    {
        Timed t(s, K_PACK_TEXELS);
        int rc = launch_pack_texels(a, s->d_packed ? packed_words(s->set_fs) : 1, s->stream);
        if (rc) return launch_status(rc, "k_pack_texels");
    }
    HIP_TRY(hipEventRecord(s->ev_tex, s->stream));
    HIP_TRY(hipStreamWaitEvent(s->setup_stream, s->ev_tex, 0));
    HIP_TRY(hipStreamWaitEvent(s->setup_stream2, s->ev_tex, 0));
    if (done) HIP_TRY(hipEventRecord(done, s->stream));
    if (other_scene) {
        HIP_TRY(hipEventRecord(s->ev_comp_done, s->stream));
        HIP_TRY(hipStreamWaitEvent(producer->stream, s->ev_comp_done, 0));
        producer->quiescent = false;
        handed_on(producer);
    }
    s->quiescent = false;
    handed_on(s);  // (rendering one of its passes again after a bin overflow would draw the new texture)
    return TR_OK;
}

// The checks the three setters share; `who` names the entry point in the error text.
int check_set_texture(const tr_scene *s, uint32_t which, uint32_t w, uint32_t h, const char *who)
{
    const std::string t(who);
    if (which > 3u) return tr::fail(TR_E_INVALID, t + ": `which` must be 0..3 (texture, normal_map, normal_map_tangent, specular_map)");
    if (w != s->tex.w[which] || h != s->tex.h[which]) {
        char buf[160];
        snprintf(buf, sizeof buf, ": the image is %u x %u, the texture it replaces %u x %u (a texture keeps its size)", w, h,
                 s->tex.w[which], s->tex.h[which]);
        return tr::fail(TR_E_INVALID, t + buf);
    }
    if (s->broken) return unusable();
    return TR_OK;
}

// A staging buffer of at least `bytes` bytes that no queued launch reads any more (a new one while all are in flight,
// up to eight; then the oldest is waited for).
int take_tex_stage(tr_scene *s, size_t bytes, tr_scene::TexStage **out)
{
    tr_scene::TexStage *free_one = nullptr;
    for (tr_scene::TexStage &t : s->tex_stage)
        if (hipEventQuery(t.done) == hipSuccess && (!free_one || (free_one->bytes < bytes && t.bytes >= bytes))) free_one = &t;
    if (!free_one && s->tex_stage.size() >= 8u) {
        free_one = &s->tex_stage.front();
        HIP_TRY(hipEventSynchronize(free_one->done));
    }
    if (!free_one) {
        tr_scene::TexStage t;
        HIP_TRY(hipEventCreateWithFlags(&t.done, hipEventDisableTiming));
        s->tex_stage.push_back(t);
        free_one = &s->tex_stage.back();
    }
    if (free_one->bytes < bytes) {
        dev_free(free_one->d);  // (idle: its event has completed, or it is new)
        free_one->bytes = 0;
        int st = dev_alloc(&free_one->d, bytes);
        if (st != TR_OK) return st;
        free_one->bytes = bytes;
    }
    *out = free_one;
    return TR_OK;
}

}  // namespace

int tr_scene_set_texture(tr_scene *s, uint32_t which, const tr_image_rgb8 *image)
{
    if (!s || !image || !image->rgb) return tr::fail(TR_E_INVALID, "tr_scene_set_texture: null argument");
    int st = check_set_texture(s, which, image->w, image->h, "tr_scene_set_texture");
    if (st != TR_OK) return st;
    HIP_TRY(hipSetDevice(s->device));
    const size_t bytes = (size_t)image->w * image->h * 3u;
    if (!s->upload_stream) HIP_TRY(hipStreamCreateWithFlags(&s->upload_stream, hipStreamNonBlocking));
    tr_scene::TexStage *stage = nullptr;
    if ((st = take_tex_stage(s, bytes, &stage)) != TR_OK) return st;
    // the copy: on a stream of its own, waited for here -- the caller's memory is free when the call returns, and the
    // copy never queues behind the scene's renders
    HIP_TRY(hipMemcpyAsync(stage->d, image->rgb, bytes, hipMemcpyHostToDevice, s->upload_stream));
    HIP_TRY(hipStreamSynchronize(s->upload_stream));
    return enqueue_pack(s, which, stage->d, nullptr, false, nullptr, stage->done);
}

int tr_scene_set_texture_device(tr_scene *s, uint32_t which, const void *rgb_device, uint32_t w, uint32_t h, tr_scene *producer)
{
    if (!s || !rgb_device) return tr::fail(TR_E_INVALID, "tr_scene_set_texture_device: null argument");
    int st = check_set_texture(s, which, w, h, "tr_scene_set_texture_device");
    if (st != TR_OK) return st;
    if (producer && producer->device != s->device)
        return tr::fail(TR_E_INVALID, "tr_scene_set_texture_device: the producer is on another device");
    if (producer && producer->broken) return unusable();
    HIP_TRY(hipSetDevice(s->device));
    const size_t bytes = (size_t)w * h * 3u;
    const void *source = nullptr;
    {
        // memory from tr_host_alloc: the kernel loads through its mapped address; else it must be device memory
        std::lock_guard<std::mutex> lock(g_host_mutex);
        auto it = g_host_allocs.find(const_cast<void *>(rgb_device));
        if (it != g_host_allocs.end()) {
            if (it->second.bytes < bytes) return tr::fail(TR_E_INVALID, "tr_scene_set_texture_device: the host buffer is smaller than the image");
            source = it->second.device;
        }
    }
    if (!source) {
        const char *text = "tr_scene_set_texture_device: `rgb_device` is neither device memory nor from tr_host_alloc "
                           "(tr_scene_set_texture takes any host memory)";
        hipPointerAttribute_t attr = {};
        if (hipPointerGetAttributes(&attr, rgb_device) != hipSuccess) {
            (void)hipGetLastError();  // (ordinary host memory is an error to the runtime: not a sticky one)
            return tr::fail(TR_E_INVALID, text);
        }
        if (attr.type != hipMemoryTypeDevice) return tr::fail(TR_E_INVALID, text);
        if (attr.device != s->device) return tr::fail(TR_E_INVALID, "tr_scene_set_texture_device: `rgb_device` is on another device");
        source = rgb_device;
    }
    if (overlaps_texels(s, source, bytes))
        return tr::fail(TR_E_INVALID, "tr_scene_set_texture_device: `rgb_device` overlaps the scene's own texel arrays");
    return enqueue_pack(s, which, (const uint8_t *)source, nullptr, false, producer, nullptr);
}

int tr_scene_set_texture_from_frame(tr_scene *dst, uint32_t which, tr_scene *src)
{
    if (!dst || !src) return tr::fail(TR_E_INVALID, "tr_scene_set_texture_from_frame: null scene");
    if (src->device != dst->device) return tr::fail(TR_E_INVALID, "tr_scene_set_texture_from_frame: the scenes are on different devices");
    if (!whole_frame(src))
        return tr::fail(TR_E_INVALID, "tr_scene_set_texture_from_frame: src is a band scene (tr_options.band_row0/1): it holds "
                                      "only its rows of the frame");
    int st = check_set_texture(dst, which, src->width, src->height, "tr_scene_set_texture_from_frame");
    if (st != TR_OK) return st;
    if (src->broken) return unusable();
    HIP_TRY(hipSetDevice(dst->device));
    // src's frame on its way (what it holds back keeps dst's old texture when src is dst); a logically cleared frame is
    // an image of zeros whatever its memory holds
    st = submit_pending(src);
    if (st != TR_OK) return st;
    return enqueue_pack(dst, which, src->d_fb, src->d_fbclean, src->z_fb_cleared, src, nullptr);
}

int tr_scene_read_texture(tr_scene *s, uint32_t which, uint8_t *rgb)
{
    if (!s || !rgb) return tr::fail(TR_E_INVALID, "tr_scene_read_texture: null argument");
    if (which > 3u) return tr::fail(TR_E_INVALID, "tr_scene_read_texture: `which` must be 0..3");
    HIP_TRY(hipSetDevice(s->device));
    int st = submit_pending(s);
    if (st != TR_OK) return st;
    HIP_TRY(hipStreamSynchronize(s->stream));
    const size_t n = (size_t)s->tex.w[which] * s->tex.h[which];
    std::vector<uint32_t> words(n);
    HIP_TRY(hipMemcpy(words.data(), s->d_texel[which], n * 4u, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; i++) {
        rgb[3 * i] = (uint8_t)words[i];
        rgb[3 * i + 1] = (uint8_t)(words[i] >> 8);
        rgb[3 * i + 2] = (uint8_t)(words[i] >> 16);
    }
    return TR_OK;
}

int tr_scene_debug_texel_set(tr_scene *s, uint32_t *words, size_t cap_words)
{
    if (!s) return tr::fail(TR_E_INVALID, "tr_scene_debug_texel_set: null scene");
    if (!s->d_packed) return 0;
    if (s->packed_count > 0x7FFFFFFFu) return tr::fail(TR_E_INVALID, "tr_scene_debug_texel_set: the set has more words than the return value holds");
    if (!words || cap_words < s->packed_count) return tr::fail(TR_E_INVALID, "tr_scene_debug_texel_set: `words` is smaller than the set");
    HIP_TRY(hipSetDevice(s->device));
    int st = submit_pending(s);
    if (st != TR_OK) return st;
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipMemcpy(words, s->d_packed, s->packed_count * 4u, hipMemcpyDeviceToHost));
    return (int)s->packed_count;
}

// The texel set tr_scene_create builds for pipeline_name from four images of one size, on the host.  Needs no GPU.
int tr_texel_set_host(const char *pipeline_name, const tr_image_rgb8 tex[4], uint32_t *words, size_t cap_words, uint32_t *blocks_per_row)
{
    if (!pipeline_name || !tex) return tr::fail(TR_E_INVALID, "tr_texel_set_host: null argument");
    const int pipe = find_pipeline(pipeline_name);
    if (pipe < 0) return tr::fail(TR_E_UNKNOWN_PIPELINE, "Provided pipeline name is not supported!");
    std::vector<uint32_t> rgba[4];
    for (int k = 0; k < 4; k++) {
        if (!tex[k].rgb || tex[k].w == 0u || tex[k].h == 0u || tex[k].w > 65535u || tex[k].h > 65535u)
            return tr::fail(TR_E_INVALID, "tr_texel_set_host: an image is missing or has a side outside 1..65535");
        if (tex[k].w != tex[0].w || tex[k].h != tex[0].h)
            return tr::fail(TR_E_INVALID, "tr_texel_set_host: the images differ in size (such a scene has no texel set)");
        const size_t n = (size_t)tex[k].w * tex[k].h;
        rgba[k].resize(n);
        for (size_t i = 0; i < n; i++) rgba[k][i] = pack_rgb8(tex[k].rgb[3 * i], tex[k].rgb[3 * i + 1], tex[k].rgb[3 * i + 2]);
    }
    const int fs = kPipelines[pipe].pass[kPipelines[pipe].n_passes - 1].fs;
    const uint32_t *const image[4] = { rgba[0].data(), rgba[1].data(), rgba[2].data(), rgba[3].data() };
    uint32_t bpr = 0;
    const std::vector<uint32_t> packed = pack_texels(fs, image, tex[0].w, tex[0].h, bpr);
    if (packed.size() > 0x7FFFFFFFu) return tr::fail(TR_E_INVALID, "tr_texel_set_host: the set has more words than the return value holds");
    if (!words || cap_words < packed.size()) return tr::fail(TR_E_INVALID, "tr_texel_set_host: `words` is smaller than the set");
    memcpy(words, packed.data(), packed.size() * 4u);
    if (blocks_per_row) *blocks_per_row = bpr;
    return (int)packed.size();
}

namespace {

// tr_ao_params as both entry points accept them (`who` names the entry point in the error text).
int check_ao_params(const tr_ao_params *p, const char *who)
{
    const std::string w(who);
    if (!p) return tr::fail(TR_E_INVALID, w + ": null argument");
    if (p->struct_size != sizeof(tr_ao_params)) return tr::fail(TR_E_INVALID, w + ": struct_size is not sizeof(tr_ao_params)");
    if (p->radius < 1u || p->radius > (uint32_t)TR_AO_MAX_RADIUS)
        return tr::fail(TR_E_INVALID, w + ": radius must be 1..TR_AO_MAX_RADIUS");
    if (p->rings < 1u || p->rings > (uint32_t)TR_AO_MAX_RINGS || p->rings > p->radius)
        return tr::fail(TR_E_INVALID, w + ": rings must be 1..TR_AO_MAX_RINGS and at most the radius");
    if (p->flags & ~TR_AO_GREY) return tr::fail(TR_E_INVALID, w + ": unknown flags");
    if (!std::isfinite(p->threshold) || p->threshold < 0.0f) return tr::fail(TR_E_INVALID, w + ": threshold must be finite and >= 0");
    if (!std::isfinite(p->falloff) || !(p->falloff > 0.0f)) return tr::fail(TR_E_INVALID, w + ": falloff must be finite and > 0");
    return TR_OK;
}

}  // namespace

static_assert(TR_AO_MAX_RADIUS == AO_MAX_RADIUS && TR_AO_MAX_RINGS == AO_MAX_RINGS && TR_AO_GREY == AO_GREY, "tr_ao.h restates the header");

int tr_scene_ambient_occlusion(tr_scene *s, const tr_ao_params *p)
{
    if (!s) return tr::fail(TR_E_INVALID, "tr_scene_ambient_occlusion: null scene");
    int st = check_ao_params(p, "tr_scene_ambient_occlusion");
    if (st != TR_OK) return st;
    if (!whole_frame(s))
        return tr::fail(TR_E_INVALID, "tr_scene_ambient_occlusion: a band scene (tr_options.band_row0/1) cannot be shaded: "
                                      "its border samples lie in another rank's rows");
    if (s->broken) return unusable();
    HIP_TRY(hipSetDevice(s->device));
    if (s->z_fb_cleared) return TR_OK;  // a logically cleared frame has no drawn pixel
    if ((st = depth_in_memory(s)) != TR_OK) return st;
    AoArgs a = {};
    a.z = s->d_z;
    a.zclean = s->d_zclean;
    a.fb = s->d_fb;
    a.fbclean = s->d_fbclean;
    a.frame = s->frame;
    a.radius = p->radius;
    a.n_taps = (uint32_t)AO_RING * p->rings;
    a.grey = (p->flags & TR_AO_GREY) ? 1u : 0u;
    a.rule = ao_rule(p->threshold, p->falloff, p->rings);
    ao_offsets(p->radius, p->rings, a.taps);
    {
        Timed t(s, K_AO);
        int rc = launch_ao(a, s->stream);
        if (rc) return launch_status(rc, "k_ao");
    }
    // (TR_AO_GREY lowers colour-clean flags of the DEVICE buffer; a record of a page-locked host buffer (HostFlags) says
    // what that host buffer holds, which this call does not change: the next read-back compares the two as always)
    s->quiescent = false;
    handed_on(s);
    return TR_OK;
}

// The rule of tr_ao.h over caller's arrays, on the host.  Needs no GPU.
int tr_ao_host(uint32_t width, uint32_t height, const float *z, uint8_t *rgb, const tr_ao_params *p)
{
    int st = check_ao_params(p, "tr_ao_host");
    if (st != TR_OK) return st;
    if (width == 0u || height == 0u) return TR_OK;
    if (!z || !rgb) return tr::fail(TR_E_INVALID, "tr_ao_host: null argument");
    ao_host(width, height, z, rgb, p->radius, p->rings, (p->flags & TR_AO_GREY) != 0u, p->threshold, p->falloff);
    return TR_OK;
}

int tr_ao_offsets(uint32_t radius, uint32_t rings, int8_t *dxdy)
{
    tr_ao_params p = { (uint32_t)sizeof(tr_ao_params), radius, rings, 0u, 1.0f, 20.0f };
    int st = check_ao_params(&p, "tr_ao_offsets");
    if (st != TR_OK) return st;
    if (!dxdy) return tr::fail(TR_E_INVALID, "tr_ao_offsets: null argument");
    AoTaps taps;
    ao_offsets(radius, rings, taps);
    memcpy(dxdy, taps.d, (size_t)2 * AO_RING * rings);
    return TR_OK;
}

namespace {

static_assert(TR_ACCUMULATE_MAX_FRAMES == ACC_MAX_FRAMES, "tr_accumulate.h restates the header");

// Frame count and weights as every accumulate entry point accepts them (`who` names the entry point in the error text;
// kept: the frames there are to choose from).  The divisor goes to *D.
int check_accumulate(uint32_t n, uint32_t kept, const uint32_t *weights, const char *who, uint32_t *D)
{
    const std::string w(who);
    if (n == 0u || n > ACC_MAX_FRAMES) return tr::fail(TR_E_INVALID, w + ": n_frames must be 1..TR_ACCUMULATE_MAX_FRAMES");
    if (n > kept)
        return tr::fail(TR_E_INVALID, w + ": more frames than the last tr_scene_render_frames call left (tr_scene_frames_kept)");
    uint32_t sum = 0;
    for (uint32_t k = 0; k < n; k++) {
        const uint32_t wk = weights ? weights[k] : 1u;
        if (wk > ACC_MAX_WEIGHT) return tr::fail(TR_E_INVALID, w + ": a weight above 255");
        sum += wk;
    }
    if (sum == 0u) return tr::fail(TR_E_INVALID, w + ": every weight is zero");
    *D = sum;
    return TR_OK;
}

// The frames the last tr_scene_render_frames call left to choose from.
uint32_t frames_kept(const tr_scene *s) { return s->last_was_group ? (uint32_t)s->tail.params.size() : 0u; }

// Enqueues the average of the last n kept frames into `out_device` (null: in place, into the current frame) behind
// everything issued so far.  n, weights and D have passed check_accumulate.
int enqueue_accumulate(tr_scene *s, uint32_t n, const uint32_t *weights, uint32_t D, uint8_t *out_device)
{
    AccumulateArgs a = {};
    bool current_is_among = false;
    for (uint32_t k = 0; k < n; k++) {
        uint8_t *fb = kept_frame_buffer(s, k);
        if (!fb) return tr::fail(TR_E_INVALID, "tr_scene_accumulate: a kept frame has no colour buffer");
        a.fb[k] = fb;
        a.w[k] = weights ? weights[k] : 1u;
        // (a set that is not remembered any more: nothing known about the buffer, every tile is read)
        for (const tr_scene::FbFlags &f : s->fb_flags)
            if (f.fb == fb) a.clean[k] = f.clean;
        current_is_among = current_is_among || fb == s->d_fb;
    }
    if (!out_device && !current_is_among)
        return tr::fail(TR_E_INVALID, "tr_scene_accumulate: in place (out == NULL) the current frame must be one of the accumulated frames");
    int st = flush_clear_color(s);  // (submits what is held back, too)
    if (st != TR_OK) return st;
    a.out = out_device ? out_device : s->d_fb;
    a.out_clean = out_device ? nullptr : s->d_fbclean;
    a.frame = s->frame;
    a.n = n;
    a.div = accumulate_divisor(D);
    return timed_launch(s, K_ACCUMULATE, "k_accumulate", [&] { return launch_accumulate(a, s->stream); });
}

}  // namespace

int tr_scene_accumulate(tr_scene *s, uint32_t n_frames, const uint32_t *weights, void *out)
{
    if (!s) return tr::fail(TR_E_INVALID, "tr_scene_accumulate: null scene");
    uint32_t D = 0;
    int st = check_accumulate(n_frames, frames_kept(s), weights, "tr_scene_accumulate", &D);
    if (st != TR_OK) return st;
    if (s->broken) return unusable();
    HIP_TRY(hipSetDevice(s->device));
    void *target = nullptr;
    st = frame_out(s, out, "tr_scene_accumulate", "tr_scene_get_accumulated", "accumulates", n_frames, &target);
    if (st == TR_OK) st = enqueue_accumulate(s, n_frames, weights, D, (uint8_t *)target);
    if (st == TR_OK) handed_on(s);
    return st;
}

int tr_scene_get_accumulated(tr_scene *s, uint32_t n_frames, const uint32_t *weights, uint8_t *rgb)
{
    if (!s) return tr::fail(TR_E_INVALID, "tr_scene_get_accumulated: null scene");
    if (!rgb) return tr::fail(TR_E_INVALID, "tr_scene_get_accumulated: null argument");
    uint32_t D = 0;
    int st = check_accumulate(n_frames, frames_kept(s), weights, "tr_scene_get_accumulated", &D);
    if (st != TR_OK) return st;
    return get_stage(s, rgb, frame_bytes(s), nullptr, [&](uint8_t *o) { return enqueue_accumulate(s, n_frames, weights, D, o); });
}

// The rule of tr_accumulate.h over caller's arrays, on the host.  Needs no GPU.
int tr_accumulate_host(size_t n_bytes, uint32_t n_frames, const uint8_t *const *frames, const uint32_t *weights, uint8_t *out)
{
    uint32_t D = 0;
    int st = check_accumulate(n_frames, n_frames, weights, "tr_accumulate_host", &D);
    if (st != TR_OK) return st;
    if (n_bytes == 0u) return TR_OK;
    if (!frames || !out) return tr::fail(TR_E_INVALID, "tr_accumulate_host: null argument");
    for (uint32_t k = 0; k < n_frames; k++)
        if (!frames[k]) return tr::fail(TR_E_INVALID, "tr_accumulate_host: null frame");
    accumulate_host(n_bytes, n_frames, frames, weights, out);
    return TR_OK;
}

namespace {

static_assert(TR_DOF_MAX_RADIUS == DOF_MAX_RADIUS && TR_DOF_SHOW_COC == DOF_SHOW_COC && sizeof(tr_dof_params) == 28, "tr_dof.h restates the header");

// tr_dof_params as every entry point accepts them (`who` names the entry point in the error text).
int check_dof_params(const tr_dof_params *p, const char *who)
{
    const std::string w(who);
    if (!p) return tr::fail(TR_E_INVALID, w + ": null argument");
    if (p->struct_size != sizeof(tr_dof_params)) return tr::fail(TR_E_INVALID, w + ": struct_size is not sizeof(tr_dof_params)");
    if (p->max_radius < 1u || p->max_radius > (uint32_t)TR_DOF_MAX_RADIUS)
        return tr::fail(TR_E_INVALID, w + ": max_radius must be 1..TR_DOF_MAX_RADIUS");
    if (p->background_radius > p->max_radius) return tr::fail(TR_E_INVALID, w + ": background_radius must be at most max_radius");
    if (p->flags & ~TR_DOF_SHOW_COC) return tr::fail(TR_E_INVALID, w + ": unknown flags");
    if (!std::isfinite(p->focus)) return tr::fail(TR_E_INVALID, w + ": focus must be finite");
    if (!std::isfinite(p->range) || p->range < 0.0f) return tr::fail(TR_E_INVALID, w + ": range must be finite and >= 0");
    if (!std::isfinite(p->scale) || !(p->scale > 0.0f)) return tr::fail(TR_E_INVALID, w + ": scale must be finite and > 0");
    return TR_OK;
}

DofRule dof_rule(const tr_dof_params *p)
{
    DofRule r;
    r.focus = p->focus;
    r.range = p->range;
    r.scale = p->scale;
    r.max_radius = p->max_radius;
    r.background_radius = p->background_radius;
    return r;
}

int check_dof_scene(const tr_scene *s, const char *who)
{
    if (!whole_frame(s))
        return tr::fail(TR_E_INVALID, std::string(who) + ": a band scene (tr_options.band_row0/1) cannot be blurred: "
                                                         "its border taps lie in another rank's rows");
    if (s->broken) return unusable();
    return TR_OK;
}

// Enqueues the blur of the current frame into `out_device` (which overlaps no frame of the scene) behind everything
// issued so far; out_clean: null, or where k_dof writes the flags of `out_device`.  The scene is not logically cleared.
int enqueue_dof(tr_scene *s, const tr_dof_params *p, uint8_t *out_device, uint32_t *out_clean)
{
    int st = depth_in_memory(s);
    if (st != TR_OK) return st;
    DofArgs a = {};
    a.z = s->d_z;
    a.zclean = s->d_zclean;
    frame_stage_args(a, s, out_device, out_clean);
    a.show_coc = (p->flags & TR_DOF_SHOW_COC) ? 1u : 0u;
    a.rule = dof_rule(p);
    return timed_launch(s, K_DOF, "k_dof", [&] { return launch_dof(a, s->stream); });
}

}  // namespace

int tr_scene_depth_of_field(tr_scene *s, const tr_dof_params *p, void *out)
{
    if (!s) return tr::fail(TR_E_INVALID, "tr_scene_depth_of_field: null scene");
    int st = check_dof_params(p, "tr_scene_depth_of_field");
    if (st == TR_OK) st = check_dof_scene(s, "tr_scene_depth_of_field");
    if (st != TR_OK) return st;
    // a logically cleared frame is black and nothing in it is drawn: zeros out of place, itself in place
    return scratch_stage(s, out, "tr_scene_depth_of_field", "tr_scene_get_depth_of_field", "blurs", true, [&](uint8_t *o, uint32_t *clean) { return enqueue_dof(s, p, o, clean); });
}

int tr_scene_get_depth_of_field(tr_scene *s, const tr_dof_params *p, uint8_t *rgb)
{
    if (!s) return tr::fail(TR_E_INVALID, "tr_scene_get_depth_of_field: null scene");
    if (!rgb) return tr::fail(TR_E_INVALID, "tr_scene_get_depth_of_field: null argument");
    int st = check_dof_params(p, "tr_scene_get_depth_of_field");
    if (st == TR_OK) st = check_dof_scene(s, "tr_scene_get_depth_of_field");
    if (st != TR_OK) return st;
    return get_scratch_stage(s, rgb, true, [&](uint8_t *o, uint32_t *clean) { return enqueue_dof(s, p, o, clean); });
}

// The rule of tr_dof.h over caller's arrays, on the host.  Needs no GPU.
int tr_dof_host(uint32_t width, uint32_t height, const float *z, const uint8_t *rgb, uint8_t *out, const tr_dof_params *p)
{
    int st = check_dof_params(p, "tr_dof_host");
    if (st != TR_OK) return st;
    if (width == 0u || height == 0u) return TR_OK;
    if (!z || !rgb || !out) return tr::fail(TR_E_INVALID, "tr_dof_host: null argument");
    if (out == rgb) return tr::fail(TR_E_INVALID, "tr_dof_host: out is rgb (the rule reads neighbours: not in place)");
    dof_host(width, height, z, rgb, out, dof_rule(p), (p->flags & TR_DOF_SHOW_COC) != 0u);
    return TR_OK;
}

int tr_dof_coc(const tr_dof_params *p, uint32_t n, const float *z, uint8_t *coc)
{
    int st = check_dof_params(p, "tr_dof_coc");
    if (st != TR_OK) return st;
    if (n == 0u) return TR_OK;
    if (!z || !coc) return tr::fail(TR_E_INVALID, "tr_dof_coc: null argument");
    dof_coc_host(dof_rule(p), n, z, coc);
    return TR_OK;
}

namespace {

static_assert(TR_BLOOM_MAX_RADIUS == BLOOM_MAX_RADIUS && TR_BLOOM_GLOW_ONLY == BLOOM_GLOW_ONLY && sizeof(tr_bloom_params) == 20,
              "tr_bloom.h restates the header");

// tr_bloom_params as every entry point accepts them (`who` names the entry point in the error text).
int check_bloom_params(const tr_bloom_params *p, const char *who)
{
    const std::string w(who);
    if (!p) return tr::fail(TR_E_INVALID, w + ": null argument");
    if (p->struct_size != sizeof(tr_bloom_params)) return tr::fail(TR_E_INVALID, w + ": struct_size is not sizeof(tr_bloom_params)");
    if (p->radius < 1u || p->radius > (uint32_t)TR_BLOOM_MAX_RADIUS) return tr::fail(TR_E_INVALID, w + ": radius must be 1..TR_BLOOM_MAX_RADIUS");
    if (p->threshold > 255u) return tr::fail(TR_E_INVALID, w + ": threshold must be 0..255");
    if (p->strength > BLOOM_MAX_STRENGTH) return tr::fail(TR_E_INVALID, w + ": strength must be 0..1024");
    if (p->flags & ~TR_BLOOM_GLOW_ONLY) return tr::fail(TR_E_INVALID, w + ": unknown flags");
    return TR_OK;
}

BloomRule bloom_rule(const tr_bloom_params *p)
{
    BloomRule r;
    r.radius = p->radius;
    r.threshold = p->threshold;
    r.strength = p->strength;
    r.glow_only = (p->flags & TR_BLOOM_GLOW_ONLY) ? 1u : 0u;
    return r;
}

int check_bloom_scene(const tr_scene *s, const char *who)
{
    if (!whole_frame(s))
        return tr::fail(TR_E_INVALID, std::string(who) + ": a band scene (tr_options.band_row0/1) cannot be bloomed: "
                                                         "its border taps lie in another rank's rows");
    if (s->broken) return unusable();
    return TR_OK;
}

// Enqueues the bloom of the current frame into `out_device` (which overlaps no frame of the scene) behind everything
// issued so far; out_clean: null, or where k_bloom writes the flags of `out_device`.  The scene is not logically cleared.
// No depth is read: a depth left on the chip stays there.
int enqueue_bloom(tr_scene *s, const tr_bloom_params *p, uint8_t *out_device, uint32_t *out_clean)
{
    int st = submit_pending(s);
    if (st != TR_OK) return st;
    BloomArgs a = {};
    frame_stage_args(a, s, out_device, out_clean);
    a.rule = bloom_rule(p);
    return timed_launch(s, K_BLOOM, "k_bloom", [&] { return launch_bloom(a, s->stream); });
}

}  // namespace

int tr_scene_bloom(tr_scene *s, const tr_bloom_params *p, void *out)
{
    if (!s) return tr::fail(TR_E_INVALID, "tr_scene_bloom: null scene");
    int st = check_bloom_params(p, "tr_scene_bloom");
    if (st == TR_OK) st = check_bloom_scene(s, "tr_scene_bloom");
    if (st != TR_OK) return st;
    // a logically cleared frame is black, and so is its glow: zeros out of place, itself in place
    return scratch_stage(s, out, "tr_scene_bloom", "tr_scene_get_bloom", "blooms", true, [&](uint8_t *o, uint32_t *clean) { return enqueue_bloom(s, p, o, clean); });
}

int tr_scene_get_bloom(tr_scene *s, const tr_bloom_params *p, uint8_t *rgb)
{
    if (!s) return tr::fail(TR_E_INVALID, "tr_scene_get_bloom: null scene");
    if (!rgb) return tr::fail(TR_E_INVALID, "tr_scene_get_bloom: null argument");
    int st = check_bloom_params(p, "tr_scene_get_bloom");
    if (st == TR_OK) st = check_bloom_scene(s, "tr_scene_get_bloom");
    if (st != TR_OK) return st;
    return get_scratch_stage(s, rgb, true, [&](uint8_t *o, uint32_t *clean) { return enqueue_bloom(s, p, o, clean); });
}

// The rule of tr_bloom.h over a caller's array, on the host.  Needs no GPU.
int tr_bloom_host(uint32_t width, uint32_t height, const uint8_t *rgb, uint8_t *out, const tr_bloom_params *p)
{
    int st = check_bloom_params(p, "tr_bloom_host");
    if (st != TR_OK) return st;
    if (width == 0u || height == 0u) return TR_OK;
    if (!rgb || !out) return tr::fail(TR_E_INVALID, "tr_bloom_host: null argument");
    if (out == rgb) return tr::fail(TR_E_INVALID, "tr_bloom_host: out is rgb (the rule reads neighbours: not in place)");
    bloom_host(width, height, rgb, out, bloom_rule(p));
    return TR_OK;
}

namespace {

static_assert(TR_GRADE_MAX_N == GRADE_MAX_N, "tr_grade.h restates the header");

int check_grade_n(uint32_t n, const char *who)
{
    if (n < 2u || n > GRADE_MAX_N) return tr::fail(TR_E_INVALID, std::string(who) + ": the table's edge n must be 2..TR_GRADE_MAX_N");
    return TR_OK;
}

int check_grade_scene(const tr_scene *s, const char *who)
{
    if (s->lut_n == 0u) return tr::fail(TR_E_INVALID, std::string(who) + ": the scene has no lookup table (tr_scene_set_lut)");
    if (s->broken) return unusable();
    return TR_OK;
}

// Does the stage short-circuit?  A logically cleared frame is black, and black maps to c0: to black where c0 is black.
bool cleared_to_black(const tr_scene *s) { return s->z_fb_cleared && s->lut_c0 == 0u; }

// Enqueues the grade of the current frame into `out_device` (null: in place) behind everything issued so far.  A
// logically cleared scene whose c0 is zero is the caller's business; with another c0 the clear is made real here and the
// kernel turns every (flagged) tile into c0.  No depth is read: a depth left on the chip stays there.
int enqueue_grade(tr_scene *s, uint8_t *out_device)
{
    int st = flush_clear_color(s);  // (submits what is held back, too)
    if (st != TR_OK) return st;
    GradeArgs a = {};
    a.fb = s->d_fb;
    a.fbclean = s->d_fbclean;
    a.out = out_device ? out_device : s->d_fb;
    a.lower_clean = (!out_device && s->lut_c0 != 0u) ? s->d_fbclean : nullptr;
    a.lut = s->d_lut;
    a.frame = s->frame;
    a.rule.n = s->lut_n;
    a.rule.c0 = s->lut_c0;
    return timed_launch(s, K_GRADE, "k_grade", [&] { return launch_grade(a, s->stream, s->grade_cap, &s->grade_grid); });
}

}  // namespace

int tr_scene_set_lut(tr_scene *s, uint32_t n, const uint8_t *lut)
{
    if (!s) return tr::fail(TR_E_INVALID, "tr_scene_set_lut: null scene");
    if (n != 0u) {
        int st = check_grade_n(n, "tr_scene_set_lut");
        if (st != TR_OK) return st;
        if (!lut) return tr::fail(TR_E_INVALID, "tr_scene_set_lut: null table");
    }
    HIP_TRY(hipSetDevice(s->device));
    // one word an entry, padded to whole 16-byte pieces (k_grade stages the table by pieces)
    const size_t entries = (size_t)n * n * n, padded = (entries + 3u) / 4u * 4u;
    std::vector<uint32_t> words(padded, 0u);
    if (n) grade_expand(n, lut, words.data());
    int st = swap_device_array(s, s->d_lut, n != 0u, words.data(), padded);
    if (st != TR_OK) return st;
    s->lut_n = n;
    s->lut_c0 = n ? words[0] : 0u;
    return TR_OK;
}

int tr_scene_grade(tr_scene *s, void *out)
{
    if (!s) return tr::fail(TR_E_INVALID, "tr_scene_grade: null scene");
    int st = check_grade_scene(s, "tr_scene_grade");
    if (st != TR_OK) return st;
    HIP_TRY(hipSetDevice(s->device));
    void *target = nullptr;
    st = frame_out(s, out, "tr_scene_grade", "tr_scene_get_graded", "grades", 0u, &target);
    if (st != TR_OK) return st;
    // zeros in the band's rows out of place, itself in place
    if (cleared_to_black(s)) return target ? cleared_out_of_place(s, target) : TR_OK;
    st = enqueue_grade(s, (uint8_t *)target);
    if (st == TR_OK) handed_on(s);
    return st;
}

int tr_scene_get_graded(tr_scene *s, uint8_t *rgb)
{
    if (!s) return tr::fail(TR_E_INVALID, "tr_scene_get_graded: null scene");
    if (!rgb) return tr::fail(TR_E_INVALID, "tr_scene_get_graded: null argument");
    int st = check_grade_scene(s, "tr_scene_get_graded");
    if (st != TR_OK) return st;
    return get_stage(s, rgb, frame_bytes(s), cleared_to_black, [&](uint8_t *o) { return enqueue_grade(s, o); });
}

// The rule of tr_grade.h over a caller's pixels, on the host.  Needs no GPU.
int tr_grade_host(size_t n_pixels, const uint8_t *rgb, uint8_t *out, uint32_t n, const uint8_t *lut)
{
    int st = check_grade_n(n, "tr_grade_host");
    if (st != TR_OK) return st;
    if (!lut) return tr::fail(TR_E_INVALID, "tr_grade_host: null table");
    if (n_pixels == 0u) return TR_OK;
    if (!rgb || !out) return tr::fail(TR_E_INVALID, "tr_grade_host: null argument");
    grade_host(n_pixels, rgb, out, n, lut);
    return TR_OK;
}

int tr_scene_debug_grade_grid(tr_scene *s, uint32_t cap)
{
    if (!s) return tr::fail(TR_E_INVALID, "tr_scene_debug_grade_grid: null scene");
    s->grade_cap = cap;
    return (int)s->grade_grid;
}

namespace {

static_assert(TR_OUTLINE_MAX_RADIUS == OUTLINE_MAX_RADIUS && TR_OUTLINE_CREASES == OUTLINE_CREASES && TR_OUTLINE_ONLY == OUTLINE_ONLY &&
                  sizeof(tr_outline_params) == 32,
              "tr_outline.h restates the header");

// tr_outline_params as every entry point accepts them (`who` names the entry point in the error text).
int check_outline_params(const tr_outline_params *p, const char *who)
{
    const std::string w(who);
    if (!p) return tr::fail(TR_E_INVALID, w + ": null argument");
    if (p->struct_size != sizeof(tr_outline_params)) return tr::fail(TR_E_INVALID, w + ": struct_size is not sizeof(tr_outline_params)");
    if (p->radius > (uint32_t)TR_OUTLINE_MAX_RADIUS) return tr::fail(TR_E_INVALID, w + ": radius must be 0..TR_OUTLINE_MAX_RADIUS");
    if (p->flags & ~(TR_OUTLINE_CREASES | TR_OUTLINE_ONLY)) return tr::fail(TR_E_INVALID, w + ": unknown flags");
    if (p->opacity > 256u) return tr::fail(TR_E_INVALID, w + ": opacity must be 0..256");
    if (p->ink[3] != 0u || p->paper[3] != 0u) return tr::fail(TR_E_INVALID, w + ": the fourth byte of ink and of paper must be 0");
    if (!std::isfinite(p->depth_step) || p->depth_step < 0.0f) return tr::fail(TR_E_INVALID, w + ": depth_step must be finite and >= 0");
    if (!std::isfinite(p->crease) || p->crease < 0.0f) return tr::fail(TR_E_INVALID, w + ": crease must be finite and >= 0");
    return TR_OK;
}

OutlineRule outline_rule(const tr_outline_params *p)
{
    OutlineRule r;
    r.radius = p->radius;
    r.flags = p->flags;
    r.opacity = p->opacity;
    r.ink = grade_pack(p->ink[0], p->ink[1], p->ink[2]);
    r.paper = grade_pack(p->paper[0], p->paper[1], p->paper[2]);
    r.depth_step = p->depth_step;
    r.crease = p->crease;
    return r;
}

int check_outline_scene(const tr_scene *s, const char *who)
{
    if (!whole_frame(s))
        return tr::fail(TR_E_INVALID, std::string(who) + ": a band scene (tr_options.band_row0/1) cannot be outlined: "
                                                         "its border neighbours lie in another rank's rows");
    if (s->broken) return unusable();
    return TR_OK;
}

// Is the stage's image of a logically cleared frame zeros?  (Under TR_OUTLINE_ONLY it is `paper`.)
bool outline_of_cleared_is_zeros(const tr_outline_params *p) { return !(p->flags & TR_OUTLINE_ONLY) || outline_rule(p).paper == 0u; }

// Enqueues the outlines of the current frame into `out_device` (null: in place) behind everything issued so far.  A
// logically cleared scene is the caller's business where its image is zeros; where it is `paper` the clear is made real
// here and the kernel turns every (flagged) tile into paper.
int enqueue_outline(tr_scene *s, const tr_outline_params *p, uint8_t *out_device)
{
    int st = s->z_fb_cleared ? flush_clear_color(s) : TR_OK;
    if (st == TR_OK) st = depth_in_memory(s);
    if (st != TR_OK) return st;
    OutlineArgs a = {};
    a.z = s->d_z;
    a.zclean = s->d_zclean;
    a.fb = s->d_fb;
    a.fbclean = s->d_fbclean;
    a.out = out_device ? out_device : s->d_fb;
    a.frame = s->frame;
    a.rule = outline_rule(p);
    return timed_launch(s, K_OUTLINE, "k_outline", [&] { return launch_outline(a, s->stream); });
}

}  // namespace

int tr_scene_outline(tr_scene *s, const tr_outline_params *p, void *out)
{
    if (!s) return tr::fail(TR_E_INVALID, "tr_scene_outline: null scene");
    int st = check_outline_params(p, "tr_scene_outline");
    if (st == TR_OK) st = check_outline_scene(s, "tr_scene_outline");
    if (st != TR_OK) return st;
    HIP_TRY(hipSetDevice(s->device));
    void *target = nullptr;
    st = frame_out(s, out, "tr_scene_outline", "tr_scene_get_outlined", "outlines", 0u, &target);
    if (st != TR_OK) return st;
    // a logically cleared frame has no drawn pixel, so no ink: itself in place; zeros, or paper, out of place
    if (s->z_fb_cleared) {
        if (!target) return TR_OK;
        if (outline_of_cleared_is_zeros(p)) return cleared_out_of_place(s, target);
    }
    st = enqueue_outline(s, p, (uint8_t *)target);
    if (st == TR_OK) handed_on(s);
    return st;
}

int tr_scene_get_outlined(tr_scene *s, const tr_outline_params *p, uint8_t *rgb)
{
    if (!s) return tr::fail(TR_E_INVALID, "tr_scene_get_outlined: null scene");
    if (!rgb) return tr::fail(TR_E_INVALID, "tr_scene_get_outlined: null argument");
    int st = check_outline_params(p, "tr_scene_get_outlined");
    if (st == TR_OK) st = check_outline_scene(s, "tr_scene_get_outlined");
    if (st != TR_OK) return st;
    return get_stage(s, rgb, frame_bytes(s), outline_of_cleared_is_zeros(p) ? cleared : nullptr,
                     [&](uint8_t *o) { return enqueue_outline(s, p, o); });
}

// The rule of tr_outline.h over caller's arrays, on the host.  Needs no GPU.
int tr_outline_host(uint32_t width, uint32_t height, const float *z, const uint8_t *rgb, uint8_t *out, const tr_outline_params *p)
{
    int st = check_outline_params(p, "tr_outline_host");
    if (st != TR_OK) return st;
    if (width == 0u || height == 0u) return TR_OK;
    if (!z || !rgb || !out) return tr::fail(TR_E_INVALID, "tr_outline_host: null argument");
    outline_host(width, height, z, rgb, out, outline_rule(p));
    return TR_OK;
}

int tr_outline_kinds(uint32_t width, uint32_t height, const float *z, const tr_outline_params *p, uint8_t *kinds)
{
    int st = check_outline_params(p, "tr_outline_kinds");
    if (st != TR_OK) return st;
    if (width == 0u || height == 0u) return TR_OK;
    if (!z || !kinds) return tr::fail(TR_E_INVALID, "tr_outline_kinds: null argument");
    outline_kinds_host(width, height, z, outline_rule(p), kinds);
    return TR_OK;
}

namespace {

static_assert(TR_AA_MAX_SEARCH == AA_MAX_SEARCH && TR_AA_SHOW_BLEND == AA_SHOW_BLEND && sizeof(tr_aa_params) == 24, "tr_aa.h restates the header");

// tr_aa_params as every entry point accepts them (`who` names the entry point in the error text).
int check_aa_params(const tr_aa_params *p, const char *who)
{
    const std::string w(who);
    if (!p) return tr::fail(TR_E_INVALID, w + ": null argument");
    if (p->struct_size != sizeof(tr_aa_params)) return tr::fail(TR_E_INVALID, w + ": struct_size is not sizeof(tr_aa_params)");
    if (p->contrast_min > 255u) return tr::fail(TR_E_INVALID, w + ": contrast_min must be 0..255");
    if (p->contrast_rel > 256u) return tr::fail(TR_E_INVALID, w + ": contrast_rel must be 0..256");
    if (p->search < 1u || p->search > (uint32_t)TR_AA_MAX_SEARCH) return tr::fail(TR_E_INVALID, w + ": search must be 1..TR_AA_MAX_SEARCH");
    if (p->subpixel > 256u) return tr::fail(TR_E_INVALID, w + ": subpixel must be 0..256");
    if (p->flags & ~TR_AA_SHOW_BLEND) return tr::fail(TR_E_INVALID, w + ": unknown flags");
    return TR_OK;
}

AaRule aa_rule(const tr_aa_params *p)
{
    AaRule r;
    r.contrast_min = p->contrast_min;
    r.contrast_rel = p->contrast_rel;
    r.search = p->search;
    r.subpixel = p->subpixel;
    r.flags = p->flags;
    return r;
}

int check_aa_scene(const tr_scene *s, const char *who)
{
    if (!whole_frame(s))
        return tr::fail(TR_E_INVALID, std::string(who) + ": a band scene (tr_options.band_row0/1) cannot be anti-aliased: "
                                                         "its border taps lie in another rank's rows");
    if (s->broken) return unusable();
    return TR_OK;
}

// Enqueues the filtered current frame into `out_device` (which overlaps no frame of the scene) behind everything issued
// so far; out_clean: null, or where k_aa writes the flags of `out_device`.  The scene is not logically cleared.  No depth
// is read: a depth left on the chip stays there.
int enqueue_aa(tr_scene *s, const tr_aa_params *p, uint8_t *out_device, uint32_t *out_clean)
{
    int st = submit_pending(s);
    if (st != TR_OK) return st;
    AaArgs a = {};
    frame_stage_args(a, s, out_device, out_clean);
    a.rule = aa_rule(p);
    return timed_launch(s, K_AA, "k_aa", [&] { return launch_aa(a, s->stream); });
}

}  // namespace

int tr_scene_antialias(tr_scene *s, const tr_aa_params *p, void *out)
{
    if (!s) return tr::fail(TR_E_INVALID, "tr_scene_antialias: null scene");
    int st = check_aa_params(p, "tr_scene_antialias");
    if (st == TR_OK) st = check_aa_scene(s, "tr_scene_antialias");
    if (st != TR_OK) return st;
    // a logically cleared frame is black and has no edge: zeros out of place, itself in place
    return scratch_stage(s, out, "tr_scene_antialias", "tr_scene_get_antialiased", "filters", true, [&](uint8_t *o, uint32_t *clean) { return enqueue_aa(s, p, o, clean); });
}

int tr_scene_get_antialiased(tr_scene *s, const tr_aa_params *p, uint8_t *rgb)
{
    if (!s) return tr::fail(TR_E_INVALID, "tr_scene_get_antialiased: null scene");
    if (!rgb) return tr::fail(TR_E_INVALID, "tr_scene_get_antialiased: null argument");
    int st = check_aa_params(p, "tr_scene_get_antialiased");
    if (st == TR_OK) st = check_aa_scene(s, "tr_scene_get_antialiased");
    if (st != TR_OK) return st;
    return get_scratch_stage(s, rgb, true, [&](uint8_t *o, uint32_t *clean) { return enqueue_aa(s, p, o, clean); });
}

// The rule of tr_aa.h over a caller's array, on the host.  Needs no GPU.
int tr_aa_host(uint32_t width, uint32_t height, const uint8_t *rgb, uint8_t *out, const tr_aa_params *p)
{
    int st = check_aa_params(p, "tr_aa_host");
    if (st != TR_OK) return st;
    if (width == 0u || height == 0u) return TR_OK;
    if (!rgb || !out) return tr::fail(TR_E_INVALID, "tr_aa_host: null argument");
    if (out == rgb) return tr::fail(TR_E_INVALID, "tr_aa_host: out is rgb (the rule reads neighbours: not in place)");
    aa_host(width, height, rgb, out, aa_rule(p));
    return TR_OK;
}

// The rule's two divisions by the inline functions of tr_aa.h, for an exhaustive check.
int tr_aa_quotients(uint32_t which, uint32_t n, const uint32_t *a, const uint32_t *b, uint32_t *out)
{
    if (which > 1u) return tr::fail(TR_E_INVALID, "tr_aa_quotients: which must be 0 (edge term) or 1 (tq)");
    if (n == 0u) return TR_OK;
    if (!a || !b || !out) return tr::fail(TR_E_INVALID, "tr_aa_quotients: null argument");
    for (uint32_t i = 0; i < n; i++) {
        const bool ok = which == 0u ? (a[i] >= 2u && a[i] <= 2u * AA_MAX_SEARCH && b[i] >= 1u && b[i] <= a[i] / 2u) : (a[i] <= 3060u && b[i] >= 1u && b[i] <= 255u);
        if (!ok) return tr::fail(TR_E_INVALID, "tr_aa_quotients: a pair outside the rule's ranges");
    }
    for (uint32_t i = 0; i < n; i++) out[i] = which == 0u ? aa_edge_offset(a[i], b[i]) : aa_tq(a[i], b[i]);
    return TR_OK;
}

namespace {

static_assert(TR_RESIZE_AREA == RESIZE_AREA && TR_RESIZE_BILINEAR == RESIZE_BILINEAR && TR_RESIZE_MAX_TAPS == RESIZE_MAX_TAPS &&
                  sizeof(tr_resize_params) == 16,
              "tr_resize.h restates the header");

// tr_resize_params as every entry point accepts them for a source of src_w x src_h pixels (`who` names the entry point
// in the error text).
int check_resize_params(const tr_resize_params *p, uint32_t src_w, uint32_t src_h, const char *who)
{
    const std::string w(who);
    if (!p) return tr::fail(TR_E_INVALID, w + ": null argument");
    if (p->flags != 0u) return tr::fail(TR_E_INVALID, w + ": flags must be 0");
    if (p->filter != TR_RESIZE_AREA && p->filter != TR_RESIZE_BILINEAR)
        return tr::fail(TR_E_INVALID, w + ": filter must be TR_RESIZE_AREA or TR_RESIZE_BILINEAR");
    if (p->width < 1u || p->width > RESIZE_MAX_SIDE || p->height < 1u || p->height > RESIZE_MAX_SIDE)
        return tr::fail(TR_E_INVALID, w + ": width and height must be 1..8192");
    if (src_w < 1u || src_h < 1u) return tr::fail(TR_E_INVALID, w + ": the source is empty");
    if (!resize_side_ok(src_w, p->width) || !resize_side_ok(src_h, p->height))
        return tr::fail(TR_E_INVALID, w + ": a side shrinks by more than 8 (width and height must be at least an eighth of the source's, rounded up)");
    return TR_OK;
}

int check_resize_scene(const tr_scene *s, const char *who)
{
    if (!whole_frame(s))
        return tr::fail(TR_E_INVALID, std::string(who) + ": a band scene (tr_options.band_row0/1) cannot be resized: "
                                                         "its border taps lie in another rank's rows");
    if (s->broken) return unusable();
    return TR_OK;
}

size_t resized_bytes(const tr_resize_params *p) { return (size_t)p->width * p->height * 3; }

// The device tables of (p->width, p->height, p->filter): the scene keeps those of its last call and builds and uploads
// others only when the key changes -- through one page-locked block, on the scene's stream, so behind every k_resize
// that still reads the old ones; the host waits for the previous upload alone before it writes the block again.
int resize_tables(tr_scene *s, const tr_resize_params *p)
{
    tr_scene::ResizeTables &t = s->resize;
    if (t.d && t.width == p->width && t.height == p->height && t.filter == p->filter) return TR_OK;
    ResizeAxis ax, ay;
    if (!ax.build(p->filter, s->width, p->width) || !ay.build(p->filter, s->height, p->height))
        return tr::fail(TR_E_INVALID, "resize: a run of taps longer than TR_RESIZE_MAX_TAPS");
    const int shape = resize_shape(ay);
    if (shape < 0) return tr::fail(TR_E_INVALID, "resize: the vertical table fits no shape of k_resize");
    // one block for every size: the weights of x, of y, then first | count << 16 of x, of y
    const size_t cap = (size_t)2 * RESIZE_MAX_SIDE * (RESIZE_MAX_TAPS * sizeof(uint16_t) + sizeof(uint32_t));
    if (!t.d) {
        int st = dev_alloc(&t.d, cap);
        if (st != TR_OK) return st;
    }
    if (!t.h) HIP_TRY(hipHostMalloc((void **)&t.h, cap, hipHostMallocDefault));
    if (!t.uploaded) HIP_TRY(hipEventCreateWithFlags(&t.uploaded, hipEventDisableTiming));
    else HIP_TRY(hipEventSynchronize(t.uploaded));
    t.width = 0u;  // (no key while the block is being rewritten: a failure below leaves no tables)
    const size_t wx = 0, wy = wx + ax.weights.size() * sizeof(uint16_t), fx = wy + ay.weights.size() * sizeof(uint16_t);
    const size_t fy = fx + (size_t)p->width * sizeof(uint32_t), bytes = fy + (size_t)p->height * sizeof(uint32_t);
    memcpy(t.h + wx, ax.weights.data(), wy - wx);
    memcpy(t.h + wy, ay.weights.data(), fx - wy);
    uint32_t *fcx = (uint32_t *)(t.h + fx), *fcy = (uint32_t *)(t.h + fy);
    for (uint32_t i = 0; i < p->width; i++) fcx[i] = (uint32_t)ax.first[i] | ((uint32_t)ax.count[i] << 16);
    for (uint32_t i = 0; i < p->height; i++) fcy[i] = (uint32_t)ay.first[i] | ((uint32_t)ay.count[i] << 16);
    HIP_TRY(hipMemcpyAsync(t.d, t.h, bytes, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipEventRecord(t.uploaded, s->stream));
    s->quiescent = false;
    t.x = { (const uint32_t *)(t.d + fx), (const uint16_t *)(t.d + wx) };
    t.y = { (const uint32_t *)(t.d + fy), (const uint16_t *)(t.d + wy) };
    t.shape = shape;
    t.y_span = ay.span((uint32_t)kResizeShapes[shape].h);
    t.x_span = ax.span((uint32_t)kResizeShapes[shape].w);
    t.width = p->width, t.height = p->height, t.filter = p->filter;
    return TR_OK;
}

// Enqueues the current frame, resized, into `out_device` (which is no frame of the scene) behind everything issued so
// far.  No depth is read: a depth left on the chip stays there.
int enqueue_resize(tr_scene *s, const tr_resize_params *p, uint8_t *out_device)
{
    int st = flush_clear_color(s);
    if (st == TR_OK) st = submit_pending(s);
    if (st == TR_OK) st = resize_tables(s, p);
    if (st != TR_OK) return st;
    ResizeArgs a = {};
    a.fb = s->d_fb;
    a.fbclean = s->d_fbclean;
    a.out = out_device;
    a.out_w = p->width;
    a.out_h = p->height;
    a.x = s->resize.x;
    a.y = s->resize.y;
    a.shape = s->resize.shape;
    a.y_span = s->resize.y_span;
    a.x_span = s->resize.x_span;
    a.frame = s->frame;
    return timed_launch(s, K_RESIZE, "k_resize", [&] { return launch_resize(a, s->stream); });
}

}  // namespace

int tr_scene_resize(tr_scene *s, const tr_resize_params *p, void *out)
{
    if (!s) return tr::fail(TR_E_INVALID, "tr_scene_resize: null scene");
    int st = check_resize_params(p, s->width, s->height, "tr_scene_resize");
    if (st == TR_OK) st = check_resize_scene(s, "tr_scene_resize");
    if (st != TR_OK) return st;
    if (!out) return tr::fail(TR_E_INVALID, "tr_scene_resize: out == NULL (the output is no frame of the scene: there is no in-place form)");
    HIP_TRY(hipSetDevice(s->device));
    void *target = nullptr;
    st = classify_out(out, resized_bytes(p), "tr_scene_resize", "tr_scene_get_resized", "resized frame", &target);
    if (st != TR_OK) return st;
    if (s->z_fb_cleared) {  // a logically cleared frame is black at every size: zeros, no kernel
        if ((st = submit_pending(s)) != TR_OK) return st;
        HIP_TRY(hipMemsetAsync(target, 0, resized_bytes(p), s->stream));
        s->quiescent = false;
    } else if ((st = enqueue_resize(s, p, (uint8_t *)target)) != TR_OK) {
        return st;
    }
    handed_on(s);
    return TR_OK;
}

int tr_scene_get_resized(tr_scene *s, const tr_resize_params *p, uint8_t *rgb)
{
    if (!s) return tr::fail(TR_E_INVALID, "tr_scene_get_resized: null scene");
    if (!rgb) return tr::fail(TR_E_INVALID, "tr_scene_get_resized: null argument");
    int st = check_resize_params(p, s->width, s->height, "tr_scene_get_resized");
    if (st == TR_OK) st = check_resize_scene(s, "tr_scene_get_resized");
    if (st != TR_OK) return st;
    return get_stage(s, rgb, resized_bytes(p), cleared, [&](uint8_t *o) { return enqueue_resize(s, p, o); });
}

// The rule of tr_resize.h over a caller's array, on the host.  Needs no GPU.
int tr_resize_host(uint32_t width, uint32_t height, const uint8_t *rgb, const tr_resize_params *p, uint8_t *out)
{
    int st = check_resize_params(p, width, height, "tr_resize_host");
    if (st != TR_OK) return st;
    if (!rgb || !out) return tr::fail(TR_E_INVALID, "tr_resize_host: null argument");
    if (out == rgb) return tr::fail(TR_E_INVALID, "tr_resize_host: out is rgb (the sizes differ and a pixel reads its neighbours: not in place)");
    if (!resize_host(width, height, rgb, p->filter, p->width, p->height, out))
        return tr::fail(TR_E_INVALID, "tr_resize_host: a run of taps longer than TR_RESIZE_MAX_TAPS");
    return TR_OK;
}

// The tables k_resize is fed for one axis, as resize_axis builds them.
int tr_resize_taps(uint32_t filter, uint32_t n_src, uint32_t n_dst, uint16_t *first, uint16_t *count, uint16_t *weights)
{
    if (filter != TR_RESIZE_AREA && filter != TR_RESIZE_BILINEAR)
        return tr::fail(TR_E_INVALID, "tr_resize_taps: filter must be TR_RESIZE_AREA or TR_RESIZE_BILINEAR");
    if (!resize_side_ok(n_src, n_dst))
        return tr::fail(TR_E_INVALID, "tr_resize_taps: n_dst must be 1..8192 and at least an eighth of n_src, rounded up");
    if (!first || !count || !weights) return tr::fail(TR_E_INVALID, "tr_resize_taps: null argument");
    if (!resize_axis(filter, n_src, n_dst, first, count, weights, nullptr))
        return tr::fail(TR_E_INVALID, "tr_resize_taps: a run of taps longer than TR_RESIZE_MAX_TAPS");
    return TR_OK;
}

namespace {

static_assert(TR_WARP_CELL == WARP_CELL && TR_WARP_BORDER == WARP_BORDER && TR_WARP_CLAMP == WARP_CLAMP &&
                  TR_WARP_PER_CHANNEL == WARP_PER_CHANNEL && sizeof(tr_warp_params) == 12,
              "tr_warp.h restates the header");

// tr_warp_params as every entry point accepts them (`who` names the entry point in the error text).
int check_warp_params(const tr_warp_params *p, const char *who)
{
    const std::string w(who);
    if (!p) return tr::fail(TR_E_INVALID, w + ": null argument");
    if (p->edge != TR_WARP_BORDER && p->edge != TR_WARP_CLAMP) return tr::fail(TR_E_INVALID, w + ": edge must be TR_WARP_BORDER or TR_WARP_CLAMP");
    if (p->pad != 0u) return tr::fail(TR_E_INVALID, w + ": pad must be 0");
    if (p->flags & ~TR_WARP_PER_CHANNEL) return tr::fail(TR_E_INVALID, w + ": unknown flags");
    return TR_OK;
}

// A grid as tr_scene_set_warp and tr_warp_host accept it: the output's size, the number of grids, every node in range.
int check_warp_grid(uint32_t width, uint32_t height, uint32_t n_grids, const int32_t *grid, const char *who)
{
    const std::string w(who);
    if (!grid) return tr::fail(TR_E_INVALID, w + ": null grid");
    if (width < 1u || width > WARP_MAX_SIDE || height < 1u || height > WARP_MAX_SIDE)
        return tr::fail(TR_E_INVALID, w + ": width and height must be 1..8192");
    if (n_grids != 1u && n_grids != 3u) return tr::fail(TR_E_INVALID, w + ": n_grids must be 1 or 3 (TR_WARP_PER_CHANNEL)");
    const size_t n = (size_t)warp_grid_side(width) * warp_grid_side(height) * 2u * n_grids;
    for (size_t i = 0; i < n; i++)
        if (grid[i] < -WARP_NODE_MAX || grid[i] > WARP_NODE_MAX)
            return tr::fail(TR_E_INVALID, w + ": a node value outside [-2^22, 2^22]");
    return TR_OK;
}

// Do the flags of a call go with the number of grids?
int check_warp_count(const tr_warp_params *p, uint32_t n_grids, const char *who)
{
    if ((p->flags & TR_WARP_PER_CHANNEL) && n_grids != 3u)
        return tr::fail(TR_E_INVALID, std::string(who) + ": TR_WARP_PER_CHANNEL needs three grids and there is one");
    if (!(p->flags & TR_WARP_PER_CHANNEL) && n_grids != 1u)
        return tr::fail(TR_E_INVALID, std::string(who) + ": three grids need TR_WARP_PER_CHANNEL");
    return TR_OK;
}

int check_warp_scene(const tr_scene *s, const tr_warp_params *p, const char *who)
{
    if (s->warp.width == 0u) return tr::fail(TR_E_INVALID, std::string(who) + ": the scene has no grid (tr_scene_set_warp)");
    int st = check_warp_count(p, s->warp.n_grids, who);
    if (st != TR_OK) return st;
    if (!whole_frame(s))
        return tr::fail(TR_E_INVALID, std::string(who) + ": a band scene (tr_options.band_row0/1) cannot be warped: "
                                                         "a pixel's source may lie in another rank's rows");
    if (s->broken) return unusable();
    return TR_OK;
}

WarpRule warp_rule(const tr_warp_params *p)
{
    WarpRule r;
    r.edge = p->edge;
    for (int c = 0; c < 3; c++) r.border[c] = p->border[c];
    r.per_channel = (p->flags & TR_WARP_PER_CHANNEL) ? 1u : 0u;
    return r;
}

size_t warped_bytes(const tr_scene *s) { return (size_t)s->warp.width * s->warp.height * 3; }

// Does the stage short-circuit?  A logically cleared frame is black, and black maps to black where no border colour
// comes in: under TR_WARP_CLAMP, or with a border of 0.
bool warp_of_cleared_is_zeros(const tr_warp_params *p) { return p->edge == TR_WARP_CLAMP || (p->border[0] | p->border[1] | p->border[2]) == 0u; }

// Enqueues the current frame, warped through the scene's grid, into `out_device` (which overlaps no frame of the
// scene) behind everything issued so far; out_clean: null, or a flag set of the frame's tile grid that is to say what
// `out_device` holds (in place: the output has the frame's size).  With another border than black a pending clear is
// made real first.  No depth is read: a depth left on the chip stays there.
int enqueue_warp(tr_scene *s, const tr_warp_params *p, uint8_t *out_device, uint32_t *out_clean)
{
    int st = flush_clear_color(s);
    if (st == TR_OK) st = submit_pending(s);
    if (st != TR_OK) return st;
    // k_warp's tiles lie 16 rows apart from the TOP, the frame's from the bottom: they are the same tiles where the
    // height is a multiple of 16, and the kernel writes the flags; otherwise every flag goes down (nothing is claimed)
    const bool same_tiles = s->height % 16u == 0u;
    if (out_clean && !same_tiles) HIP_TRY(hipMemsetAsync(out_clean, 0, (size_t)s->n_tiles * 4, s->stream));
    WarpArgs a = {};
    frame_stage_args(a, s, out_device, same_tiles ? out_clean : nullptr);
    a.grid = s->warp.d;
    a.out_w = s->warp.width;
    a.out_h = s->warp.height;
    a.rule = warp_rule(p);
    return timed_launch(s, K_WARP, "k_warp", [&] { return launch_warp(a, s->stream); });
}

}  // namespace

int tr_scene_set_warp(tr_scene *s, uint32_t width, uint32_t height, uint32_t n_grids, const int32_t *grid)
{
    if (!s) return tr::fail(TR_E_INVALID, "tr_scene_set_warp: null scene");
    int st = check_warp_grid(width, height, n_grids, grid, "tr_scene_set_warp");
    if (st != TR_OK) return st;
    HIP_TRY(hipSetDevice(s->device));
    tr_scene::WarpGrid &g = s->warp;
    const size_t n = (size_t)warp_grid_side(width) * warp_grid_side(height) * 2u * n_grids;
    if (!g.uploaded) HIP_TRY(hipEventCreateWithFlags(&g.uploaded, hipEventDisableTiming));
    if (g.cap < n) {
        // larger blocks: a k_warp issued earlier may still read the old device block, so the stream runs empty first
        int32_t *d_new = nullptr, *h_new = nullptr;
        if ((st = dev_alloc(&d_new, n)) != TR_OK) return st;
        if (hipHostMalloc((void **)&h_new, n * sizeof(int32_t), hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            dev_free(d_new);
            return tr::fail(TR_E_NOMEM, "tr_scene_set_warp: no page-locked memory for the grid");
        }
        hipError_t e = hipStreamSynchronize(s->stream);
        if (e != hipSuccess) {
            dev_free(d_new);
            (void)hipHostFree(h_new);
            HIP_TRY(e);
        }
        dev_free(g.d);
        if (g.h) (void)hipHostFree(g.h);
        g.d = d_new, g.h = h_new, g.cap = n;
        g.width = 0u;
    } else {
        HIP_TRY(hipEventSynchronize(g.uploaded));  // (the previous upload has left the page-locked block)
    }
    g.width = 0u;  // (no grid while the block is being rewritten: a failure below leaves none)
    memcpy(g.h, grid, n * sizeof(int32_t));
    // in stream order: behind every k_warp that still reads the old nodes
    HIP_TRY(hipMemcpyAsync(g.d, g.h, n * sizeof(int32_t), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipEventRecord(g.uploaded, s->stream));
    s->quiescent = false;
    g.width = width, g.height = height, g.n_grids = n_grids;
    return TR_OK;
}

int tr_scene_warp(tr_scene *s, const tr_warp_params *p, void *out)
{
    if (!s) return tr::fail(TR_E_INVALID, "tr_scene_warp: null scene");
    int st = check_warp_params(p, "tr_scene_warp");
    if (st == TR_OK) st = check_warp_scene(s, p, "tr_scene_warp");
    if (st != TR_OK) return st;
    if (!out && (s->warp.width != s->width || s->warp.height != s->height))
        return tr::fail(TR_E_INVALID, "tr_scene_warp: out == NULL warps in place, and the grid's size is not the frame's");
    HIP_TRY(hipSetDevice(s->device));
    void *target = nullptr;
    if (out) {
        st = classify_out(out, warped_bytes(s), "tr_scene_warp", "tr_scene_get_warped", "warped frame", &target);
        if (st == TR_OK) st = refuse_overlap(s, target, frame_bytes(s), "tr_scene_warp", "warps", 0u, warped_bytes(s));
        if (st != TR_OK) return st;
    }
    // a logically cleared frame is black, and so is its warp where no border colour comes in: zeros out of place,
    // itself in place
    if (s->z_fb_cleared && warp_of_cleared_is_zeros(p)) {
        if (!target) return TR_OK;
        if ((st = submit_pending(s)) != TR_OK) return st;
        HIP_TRY(hipMemsetAsync(target, 0, warped_bytes(s), s->stream));
        s->quiescent = false;
        handed_on(s);
        return TR_OK;
    }
    auto enqueue = [&](uint8_t *o, uint32_t *clean) { return enqueue_warp(s, p, o, clean); };
    st = target ? enqueue((uint8_t *)target, nullptr) : in_place_via_scratch(s, enqueue);
    if (st == TR_OK) handed_on(s);
    return st;
}

int tr_scene_get_warped(tr_scene *s, const tr_warp_params *p, uint8_t *rgb)
{
    if (!s) return tr::fail(TR_E_INVALID, "tr_scene_get_warped: null scene");
    if (!rgb) return tr::fail(TR_E_INVALID, "tr_scene_get_warped: null argument");
    int st = check_warp_params(p, "tr_scene_get_warped");
    if (st == TR_OK) st = check_warp_scene(s, p, "tr_scene_get_warped");
    if (st != TR_OK) return st;
    // (the predicate takes the scene alone: the parameters decide here which one is asked)
    return get_stage(s, rgb, warped_bytes(s), warp_of_cleared_is_zeros(p) ? cleared : nullptr,
                     [&](uint8_t *o) { return enqueue_warp(s, p, o, nullptr); });
}

// The rule of tr_warp.h over a caller's array, on the host.  Needs no GPU.
int tr_warp_host(uint32_t width, uint32_t height, const uint8_t *rgb, uint32_t out_width, uint32_t out_height, uint32_t n_grids,
                 const int32_t *grid, const tr_warp_params *p, uint8_t *out)
{
    int st = check_warp_params(p, "tr_warp_host");
    if (st == TR_OK) st = check_warp_grid(out_width, out_height, n_grids, grid, "tr_warp_host");
    if (st == TR_OK) st = check_warp_count(p, n_grids, "tr_warp_host");
    if (st != TR_OK) return st;
    if (width < 1u || height < 1u) return tr::fail(TR_E_INVALID, "tr_warp_host: the source is empty");
    if (!rgb || !out) return tr::fail(TR_E_INVALID, "tr_warp_host: null argument");
    if (out == rgb) return tr::fail(TR_E_INVALID, "tr_warp_host: out is rgb (a pixel reads other pixels: not in place)");
    warp_host(width, height, rgb, out_width, out_height, grid, warp_rule(p), out);
    return TR_OK;
}

namespace {

static_assert(TR_CONVOLVE_SEPARABLE == CONVOLVE_SEPARABLE && TR_CONVOLVE_ABS == CONVOLVE_ABS && TR_CONVOLVE_UNSHARP == CONVOLVE_UNSHARP &&
                  TR_CONVOLVE_BORDER == CONVOLVE_BORDER && TR_CONVOLVE_CLAMP == CONVOLVE_CLAMP && sizeof(tr_convolve_params) == 200 &&
                  sizeof(((tr_convolve_params *)nullptr)->weights) == CONVOLVE_MAX_WEIGHTS * sizeof(int16_t),
              "tr_convolve.h restates the header");

// tr_convolve_params as every entry point accepts them (`who` names the entry point in the error text).
int check_convolve_params(const tr_convolve_params *p, const char *who)
{
    const std::string w(who);
    if (!p) return tr::fail(TR_E_INVALID, w + ": null argument");
    if (p->struct_size != sizeof(tr_convolve_params)) return tr::fail(TR_E_INVALID, w + ": struct_size is not sizeof(tr_convolve_params)");
    if (p->flags & ~(TR_CONVOLVE_SEPARABLE | TR_CONVOLVE_ABS | TR_CONVOLVE_UNSHARP)) return tr::fail(TR_E_INVALID, w + ": unknown flags");
    const bool sep = (p->flags & TR_CONVOLVE_SEPARABLE) != 0u, unsharp = (p->flags & TR_CONVOLVE_UNSHARP) != 0u;
    const uint32_t k_max = sep ? (uint32_t)CONVOLVE_MAX_SEPARABLE : (uint32_t)CONVOLVE_MAX_GENERAL;
    if (p->kw % 2u == 0u || p->kh % 2u == 0u || p->kw > k_max || p->kh > k_max)
        return tr::fail(TR_E_INVALID, w + (sep ? ": kw and kh must be odd and 1..31 (TR_CONVOLVE_SEPARABLE)" : ": kw and kh must be odd and 1..9 (1..31 with TR_CONVOLVE_SEPARABLE)"));
    if (p->shift > CONVOLVE_MAX_SHIFT) return tr::fail(TR_E_INVALID, w + ": shift must be 0..22");
    if (p->bias < -CONVOLVE_MAX_BIAS || p->bias > CONVOLVE_MAX_BIAS) return tr::fail(TR_E_INVALID, w + ": bias must be -255..255");
    if (p->amount > CONVOLVE_MAX_AMOUNT) return tr::fail(TR_E_INVALID, w + ": amount must be 0..1024");
    if (!unsharp && p->amount != 0u) return tr::fail(TR_E_INVALID, w + ": amount must be 0 without TR_CONVOLVE_UNSHARP");
    if (p->edge != TR_CONVOLVE_BORDER && p->edge != TR_CONVOLVE_CLAMP) return tr::fail(TR_E_INVALID, w + ": edge must be TR_CONVOLVE_BORDER or TR_CONVOLVE_CLAMP");
    if (p->pad != 0u) return tr::fail(TR_E_INVALID, w + ": pad must be 0");
    auto sum_abs = [&](uint32_t first, uint32_t n) {
        int64_t a = 0;
        for (uint32_t i = 0; i < n; i++) a += std::abs((int64_t)p->weights[first + i]);
        return a;
    };
    const int64_t row = sep ? sum_abs(0u, p->kw) : 0;
    const int64_t A = sep ? row * sum_abs(p->kw, p->kh) : sum_abs(0u, p->kw * p->kh);
    if (A > CONVOLVE_MAX_A) return tr::fail(TR_E_INVALID, w + ": the weights' absolute sum exceeds 2^22 (separable: the product of the row's and the column's)");
    if (row > CONVOLVE_MAX_ROW) return tr::fail(TR_E_INVALID, w + ": the row's absolute sum exceeds 2^15");
    if (unsharp && (p->flags & TR_CONVOLVE_ABS)) return tr::fail(TR_E_INVALID, w + ": TR_CONVOLVE_UNSHARP does not go with TR_CONVOLVE_ABS");
    if (unsharp && p->bias != 0) return tr::fail(TR_E_INVALID, w + ": TR_CONVOLVE_UNSHARP needs a bias of 0");
    return TR_OK;
}

ConvolveRule convolve_rule(const tr_convolve_params *p)
{
    ConvolveRule r = {};
    r.kw = p->kw, r.kh = p->kh, r.flags = p->flags, r.shift = p->shift, r.bias = p->bias, r.amount = p->amount, r.edge = p->edge;
    r.border = (uint32_t)p->border[0] | ((uint32_t)p->border[1] << 8) | ((uint32_t)p->border[2] << 16);
    const uint32_t n = (p->flags & TR_CONVOLVE_SEPARABLE) ? p->kw + p->kh : p->kw * p->kh;
    for (uint32_t i = 0; i < n; i++) r.weights[i] = p->weights[i];  // (entries behind the last one used are not read)
    return r;
}

// The scene as the neighbourhood stages (convolve, rank, bilateral) accept it; `verb`: "convolved", "ranked", "smoothed".
int check_neigh_scene(const tr_scene *s, const char *who, const char *verb)
{
    if (!whole_frame(s))
        return tr::fail(TR_E_INVALID, std::string(who) + ": a band scene (tr_options.band_row0/1) cannot be " + verb + ": "
                                                         "its border taps lie in another rank's rows");
    if (s->broken) return unusable();
    return TR_OK;
}

// Is the rule's image of a black frame black?  The constant of a neighbourhood of zeros is 0, and no border colour
// comes in: TR_CONVOLVE_CLAMP, or a border of 0.
bool convolve_of_black_is_black(const tr_convolve_params *p)
{
    return convolve_of_zeros(convolve_rule(p)) == 0u && (p->edge == TR_CONVOLVE_CLAMP || (p->border[0] | p->border[1] | p->border[2]) == 0u);
}

// Enqueues the current frame, filtered, into `out_device` (which overlaps no frame of the scene) behind everything
// issued so far; out_clean: null, or where k_convolve writes the flags of `out_device`.  A pending clear is made real
// first.  No depth is read: a depth left on the chip stays there.
int enqueue_convolve(tr_scene *s, const tr_convolve_params *p, uint8_t *out_device, uint32_t *out_clean)
{
    int st = flush_clear_color(s);
    if (st == TR_OK) st = submit_pending(s);
    if (st != TR_OK) return st;
    ConvolveArgs a = {};
    frame_stage_args(a, s, out_device, out_clean);
    a.rule = convolve_rule(p);
    return timed_launch(s, K_CONVOLVE, "k_convolve", [&] { return launch_convolve(a, s->stream); });
}

}  // namespace

int tr_scene_convolve(tr_scene *s, const tr_convolve_params *p, void *out)
{
    if (!s) return tr::fail(TR_E_INVALID, "tr_scene_convolve: null scene");
    int st = check_convolve_params(p, "tr_scene_convolve");
    if (st == TR_OK) st = check_neigh_scene(s, "tr_scene_convolve", "convolved");
    if (st != TR_OK) return st;
    // a logically cleared frame is black, and so is its image where the rule gives black: zeros out of place, itself in place
    return scratch_stage(s, out, "tr_scene_convolve", "tr_scene_get_convolved", "convolves", convolve_of_black_is_black(p), [&](uint8_t *o, uint32_t *clean) { return enqueue_convolve(s, p, o, clean); });
}

int tr_scene_get_convolved(tr_scene *s, const tr_convolve_params *p, uint8_t *rgb)
{
    if (!s) return tr::fail(TR_E_INVALID, "tr_scene_get_convolved: null scene");
    if (!rgb) return tr::fail(TR_E_INVALID, "tr_scene_get_convolved: null argument");
    int st = check_convolve_params(p, "tr_scene_get_convolved");
    if (st == TR_OK) st = check_neigh_scene(s, "tr_scene_get_convolved", "convolved");
    if (st != TR_OK) return st;
    return get_scratch_stage(s, rgb, convolve_of_black_is_black(p), [&](uint8_t *o, uint32_t *clean) { return enqueue_convolve(s, p, o, clean); });
}

// The rule of tr_convolve.h over a caller's array, on the host.  Needs no GPU.
int tr_convolve_host(uint32_t width, uint32_t height, const uint8_t *rgb, uint8_t *out, const tr_convolve_params *p)
{
    int st = check_convolve_params(p, "tr_convolve_host");
    if (st != TR_OK) return st;
    if (width == 0u || height == 0u) return TR_OK;
    if (!rgb || !out) return tr::fail(TR_E_INVALID, "tr_convolve_host: null argument");
    if (out == rgb) return tr::fail(TR_E_INVALID, "tr_convolve_host: out is rgb (the rule reads neighbours: not in place)");
    convolve_host(width, height, rgb, out, convolve_rule(p));
    return TR_OK;
}

namespace {

static_assert(TR_RANK_VALUE == RANK_VALUE && TR_RANK_RANGE == RANK_RANGE && TR_RANK_MID == RANK_MID && TR_RANK_CLAMP_CENTRE == RANK_CLAMP_CENTRE &&
                  TR_RANK_BORDER == RANK_BORDER && TR_RANK_CLAMP == RANK_CLAMP && sizeof(tr_rank_params) == 64 && sizeof(RankParams) == sizeof(tr_rank_params) &&
                  offsetof(tr_rank_params, edge) == offsetof(RankParams, edge) && offsetof(tr_rank_params, border) == offsetof(RankParams, border) &&
                  offsetof(tr_rank_params, pad) == offsetof(RankParams, pad) && offsetof(tr_rank_params, rows) == offsetof(RankParams, rows) &&
                  offsetof(tr_rank_params, pad2) == offsetof(RankParams, pad2),
              "tr_rank.h restates the header");

// tr_rank_params as every entry point accepts them (`who` names the entry point in the error text); *q: tr_rank.h's copy.
int check_rank_params(const tr_rank_params *p, const char *who, RankParams *q)
{
    if (!p) return tr::fail(TR_E_INVALID, std::string(who) + ": null argument");
    memcpy(q, p, sizeof(RankParams));
    const char *why = rank_refusal(*q);
    return why ? tr::fail(TR_E_INVALID, std::string(who) + why) : TR_OK;
}

// Is the rule's image of a black frame black?  A neighbourhood of zeros is 0 under every op, so: no border colour comes
// in -- TR_RANK_CLAMP, or a border of 0.
bool rank_of_black_is_black(const RankParams &q) { return q.edge == RANK_CLAMP || (q.border[0] | q.border[1] | q.border[2]) == 0u; }

// Enqueues the current frame, filtered, into `out_device` (which overlaps no frame of the scene) behind everything
// issued so far; out_clean: null, or where k_rank writes the flags of `out_device`.  A pending clear is made real
// first.  No depth is read: a depth left on the chip stays there.
int enqueue_rank(tr_scene *s, const RankParams &q, uint8_t *out_device, uint32_t *out_clean)
{
    int st = flush_clear_color(s);
    if (st == TR_OK) st = submit_pending(s);
    if (st != TR_OK) return st;
    RankArgs a = {};
    frame_stage_args(a, s, out_device, out_clean);
    a.rule = rank_rule(q);
    return timed_launch(s, K_RANK, "k_rank", [&] { return launch_rank(a, s->stream); });
}

}  // namespace

int tr_scene_rank(tr_scene *s, const tr_rank_params *p, void *out)
{
    if (!s) return tr::fail(TR_E_INVALID, "tr_scene_rank: null scene");
    RankParams q;
    int st = check_rank_params(p, "tr_scene_rank", &q);
    if (st == TR_OK) st = check_neigh_scene(s, "tr_scene_rank", "ranked");
    if (st != TR_OK) return st;
    // a logically cleared frame is black, and so is its image where no border colour comes in: zeros out of place, itself in place
    return scratch_stage(s, out, "tr_scene_rank", "tr_scene_get_ranked", "ranks", rank_of_black_is_black(q), [&](uint8_t *o, uint32_t *clean) { return enqueue_rank(s, q, o, clean); });
}

int tr_scene_get_ranked(tr_scene *s, const tr_rank_params *p, uint8_t *rgb)
{
    if (!s) return tr::fail(TR_E_INVALID, "tr_scene_get_ranked: null scene");
    if (!rgb) return tr::fail(TR_E_INVALID, "tr_scene_get_ranked: null argument");
    RankParams q;
    int st = check_rank_params(p, "tr_scene_get_ranked", &q);
    if (st == TR_OK) st = check_neigh_scene(s, "tr_scene_get_ranked", "ranked");
    if (st != TR_OK) return st;
    return get_scratch_stage(s, rgb, rank_of_black_is_black(q), [&](uint8_t *o, uint32_t *clean) { return enqueue_rank(s, q, o, clean); });
}

// The rule of tr_rank.h over a caller's array, on the host.  Needs no GPU.
int tr_rank_host(uint32_t width, uint32_t height, const uint8_t *rgb, uint8_t *out, const tr_rank_params *p)
{
    RankParams q;
    int st = check_rank_params(p, "tr_rank_host", &q);
    if (st != TR_OK) return st;
    if (width == 0u || height == 0u) return TR_OK;
    if (!rgb || !out) return tr::fail(TR_E_INVALID, "tr_rank_host: null argument");
    if (out == rgb) return tr::fail(TR_E_INVALID, "tr_rank_host: out is rgb (the rule reads neighbours: not in place)");
    rank_host(width, height, rgb, out, rank_rule(q));
    return TR_OK;
}

namespace {

static_assert(TR_BILATERAL_GUIDE_COLOUR == BILATERAL_GUIDE_COLOUR && TR_BILATERAL_GUIDE_DEPTH == BILATERAL_GUIDE_DEPTH && TR_BILATERAL_BORDER == BILATERAL_BORDER &&
                  TR_BILATERAL_CLAMP == BILATERAL_CLAMP && sizeof(tr_bilateral_params) == 512 && sizeof(BilateralParams) == sizeof(tr_bilateral_params) &&
                  offsetof(tr_bilateral_params, edge) == offsetof(BilateralParams, edge) && offsetof(tr_bilateral_params, depth_scale) == offsetof(BilateralParams, depth_scale) &&
                  offsetof(tr_bilateral_params, border) == offsetof(BilateralParams, border) && offsetof(tr_bilateral_params, pad) == offsetof(BilateralParams, pad) &&
                  offsetof(tr_bilateral_params, spatial) == offsetof(BilateralParams, spatial) && offsetof(tr_bilateral_params, pad2) == offsetof(BilateralParams, pad2) &&
                  offsetof(tr_bilateral_params, range) == offsetof(BilateralParams, range),
              "tr_bilateral.h restates the header");

// tr_bilateral_params as every entry point accepts them (`who` names the entry point in the error text); *q: tr_bilateral.h's copy.
int check_bilateral_params(const tr_bilateral_params *p, const char *who, BilateralParams *q)
{
    if (!p) return tr::fail(TR_E_INVALID, std::string(who) + ": null argument");
    memcpy(q, p, sizeof(BilateralParams));
    const char *why = bilateral_refusal(*q);
    return why ? tr::fail(TR_E_INVALID, std::string(who) + why) : TR_OK;
}

// Is the rule's image of a black frame black?  A weighted mean of zeros is 0 and S == 0 gives the centre, which is 0 too,
// under both guides, so: no border colour comes in -- TR_BILATERAL_CLAMP, or a border of 0.
bool bilateral_of_black_is_black(const BilateralParams &q) { return q.edge == BILATERAL_CLAMP || (q.border[0] | q.border[1] | q.border[2]) == 0u; }

// Enqueues the current frame, filtered, into `out_device` (which overlaps no frame of the scene) behind everything
// issued so far; out_clean: null, or where k_bilateral writes the flags of `out_device`.  A pending clear is made real
// first.  The DEPTH guide reads the depth, which is made real; the COLOUR guide reads none: a depth left on the chip
// stays there.
int enqueue_bilateral(tr_scene *s, const BilateralParams &q, uint8_t *out_device, uint32_t *out_clean)
{
    const bool depth = q.guide == BILATERAL_GUIDE_DEPTH;
    int st = flush_clear_color(s);
    if (st == TR_OK) st = submit_pending(s);
    if (st == TR_OK && depth) st = depth_in_memory(s);
    if (st != TR_OK) return st;
    BilateralArgs a = {};
    if (depth) a.z = s->d_z, a.zclean = s->d_zclean;
    frame_stage_args(a, s, out_device, out_clean);
    a.rule = bilateral_rule(q);
    return timed_launch(s, K_BILATERAL, "k_bilateral", [&] { return launch_bilateral(a, s->stream); });
}

}  // namespace

int tr_scene_bilateral(tr_scene *s, const tr_bilateral_params *p, void *out)
{
    if (!s) return tr::fail(TR_E_INVALID, "tr_scene_bilateral: null scene");
    BilateralParams q;
    int st = check_bilateral_params(p, "tr_scene_bilateral", &q);
    if (st == TR_OK) st = check_neigh_scene(s, "tr_scene_bilateral", "smoothed");
    if (st != TR_OK) return st;
    // a logically cleared frame is black, and so is its image where no border colour comes in: zeros out of place, itself in place
    return scratch_stage(s, out, "tr_scene_bilateral", "tr_scene_get_bilateral", "smooths", bilateral_of_black_is_black(q), [&](uint8_t *o, uint32_t *clean) { return enqueue_bilateral(s, q, o, clean); });
}

int tr_scene_get_bilateral(tr_scene *s, const tr_bilateral_params *p, uint8_t *rgb)
{
    if (!s) return tr::fail(TR_E_INVALID, "tr_scene_get_bilateral: null scene");
    if (!rgb) return tr::fail(TR_E_INVALID, "tr_scene_get_bilateral: null argument");
    BilateralParams q;
    int st = check_bilateral_params(p, "tr_scene_get_bilateral", &q);
    if (st == TR_OK) st = check_neigh_scene(s, "tr_scene_get_bilateral", "smoothed");
    if (st != TR_OK) return st;
    return get_scratch_stage(s, rgb, bilateral_of_black_is_black(q), [&](uint8_t *o, uint32_t *clean) { return enqueue_bilateral(s, q, o, clean); });
}

// The rule of tr_bilateral.h over a caller's arrays, on the host.  Needs no GPU.
int tr_bilateral_host(uint32_t width, uint32_t height, const uint8_t *rgb, const float *z, uint8_t *out, const tr_bilateral_params *p)
{
    BilateralParams q;
    int st = check_bilateral_params(p, "tr_bilateral_host", &q);
    if (st != TR_OK) return st;
    if (width == 0u || height == 0u) return TR_OK;
    if (!rgb || !out || (!z && q.guide == BILATERAL_GUIDE_DEPTH)) return tr::fail(TR_E_INVALID, "tr_bilateral_host: null argument");
    if (out == rgb) return tr::fail(TR_E_INVALID, "tr_bilateral_host: out is rgb (the rule reads neighbours: not in place)");
    bilateral_host(width, height, rgb, z, out, bilateral_rule(q));
    return TR_OK;
}

namespace {

static_assert(TR_YUV_I420 == YUV_I420 && TR_YUV_NV12 == YUV_NV12 && TR_YUV_I444 == YUV_I444 && TR_YUV_BT601 == YUV_BT601 &&
                  TR_YUV_BT709 == YUV_BT709 && TR_YUV_FULL == YUV_FULL && TR_YUV_LIMITED == YUV_LIMITED && sizeof(tr_yuv_params) == 16,
              "tr_yuv.h restates the header");

// tr_yuv_params as every entry point accepts them (`who` names the entry point in the error text).
int check_yuv_params(const tr_yuv_params *p, const char *who)
{
    const std::string w(who);
    if (!p) return tr::fail(TR_E_INVALID, w + ": null argument");
    if (p->flags != 0u) return tr::fail(TR_E_INVALID, w + ": flags must be 0");
    if (!yuv_layout_ok(p->layout)) return tr::fail(TR_E_INVALID, w + ": layout must be TR_YUV_I420, TR_YUV_NV12 or TR_YUV_I444");
    if (p->matrix != TR_YUV_BT601 && p->matrix != TR_YUV_BT709) return tr::fail(TR_E_INVALID, w + ": matrix must be TR_YUV_BT601 or TR_YUV_BT709");
    if (p->range != TR_YUV_FULL && p->range != TR_YUV_LIMITED) return tr::fail(TR_E_INVALID, w + ": range must be TR_YUV_FULL or TR_YUV_LIMITED");
    return TR_OK;
}

int check_yuv_size(uint32_t width, uint32_t height, const char *who)
{
    if (width < 1u || width > YUV_MAX_SIDE || height < 1u || height > YUV_MAX_SIDE)
        return tr::fail(TR_E_INVALID, std::string(who) + ": width and height must be 1..8192");
    return TR_OK;
}

int check_yuv_scene(const tr_scene *s, const char *who)
{
    if (!whole_frame(s))
        return tr::fail(TR_E_INVALID, std::string(who) + ": a band scene (tr_options.band_row0/1) cannot be converted: "
                                                         "a chroma sample's pair of rows straddles a band's border, and its planes are not the frame's rows");
    if (s->broken) return unusable();
    return TR_OK;
}

YuvRule yuv_rule(const tr_yuv_params *p)
{
    YuvRule k = kYuvTables[p->matrix][p->range];
    k.layout = p->layout;
    return k;
}

// The planes of black -- Y = y0, chroma 128 -- into `out_device` by fills behind everything issued so far: no kernel.
int fill_yuv_black(tr_scene *s, uint32_t width, uint32_t height, const tr_yuv_params *p, uint8_t *out_device)
{
    const size_t wh = (size_t)width * height, all = yuv_bytes(width, height, p->layout);
    HIP_TRY(hipMemsetAsync(out_device, kYuvTables[p->matrix][p->range].y0, wh, s->stream));
    HIP_TRY(hipMemsetAsync(out_device + wh, 128, all - wh, s->stream));
    s->quiescent = false;
    return TR_OK;
}

// Enqueues the conversion of src (width x height, with its flags or null) into `out_device` on the scene's stream.
int launch_yuv_on(tr_scene *s, const uint8_t *src, const uint32_t *clean, uint32_t width, uint32_t height, const tr_yuv_params *p, uint8_t *out_device)
{
    YuvArgs a = {};
    a.src = src;
    a.clean = clean;
    a.out = out_device;
    a.width = width;
    a.height = height;
    a.ntx = (width + (uint32_t)TILE_W - 1u) / (uint32_t)TILE_W;
    a.rule = yuv_rule(p);
    return timed_launch(s, K_YUV, "k_yuv", [&] { return launch_yuv(a, s->stream); });
}

// Enqueues the current frame's planes into `out_device` (which is no frame of the scene) behind everything issued so
// far; a logically cleared scene gives the black planes by fills.  No depth is read: a depth left on the chip stays there.
int enqueue_yuv(tr_scene *s, const tr_yuv_params *p, uint8_t *out_device)
{
    if (s->z_fb_cleared) {
        int st = submit_pending(s);
        return st != TR_OK ? st : fill_yuv_black(s, s->width, s->height, p, out_device);
    }
    int st = flush_clear_color(s);
    if (st == TR_OK) st = submit_pending(s);
    if (st != TR_OK) return st;
    return launch_yuv_on(s, s->d_fb, s->d_fbclean, s->width, s->height, p, out_device);
}

}  // namespace

int tr_scene_to_yuv(tr_scene *s, const tr_yuv_params *p, void *out)
{
    if (!s) return tr::fail(TR_E_INVALID, "tr_scene_to_yuv: null scene");
    int st = check_yuv_params(p, "tr_scene_to_yuv");
    if (st == TR_OK) st = check_yuv_size(s->width, s->height, "tr_scene_to_yuv");
    if (st == TR_OK) st = check_yuv_scene(s, "tr_scene_to_yuv");
    if (st != TR_OK) return st;
    if (!out) return tr::fail(TR_E_INVALID, "tr_scene_to_yuv: out == NULL (the planes are no frame of the scene: there is no in-place form)");
    HIP_TRY(hipSetDevice(s->device));
    void *target = nullptr;
    const size_t bytes = yuv_bytes(s->width, s->height, p->layout);
    st = classify_out(out, bytes, "tr_scene_to_yuv", "tr_scene_get_yuv", "planes", &target);
    if (st != TR_OK) return st;
    if (refuse_overlap(s, target, frame_bytes(s), "tr_scene_to_yuv", "converts", 0u, bytes) != TR_OK)
        return tr::fail(TR_E_INVALID, "tr_scene_to_yuv: `out` overlaps a frame buffer of the scene (there is no in-place form)");
    if ((st = enqueue_yuv(s, p, (uint8_t *)target)) != TR_OK) return st;
    handed_on(s);
    return TR_OK;
}

int tr_scene_to_yuv_from(tr_scene *s, const void *rgb, uint32_t width, uint32_t height, const tr_yuv_params *p, void *out)
{
    if (!s) return tr::fail(TR_E_INVALID, "tr_scene_to_yuv_from: null scene");
    if (!rgb) return tr::fail(TR_E_INVALID, "tr_scene_to_yuv_from: null argument");
    int st = check_yuv_params(p, "tr_scene_to_yuv_from");
    if (st == TR_OK) st = check_yuv_size(width, height, "tr_scene_to_yuv_from");
    if (st != TR_OK) return st;
    if (s->broken) return unusable();
    if (!out) return tr::fail(TR_E_INVALID, "tr_scene_to_yuv_from: out == NULL (there is no in-place form)");
    HIP_TRY(hipSetDevice(s->device));
    const size_t in_bytes = (size_t)width * height * 3u, bytes = yuv_bytes(width, height, p->layout);
    const void *source = nullptr;
    {
        // memory from tr_host_alloc: the kernel loads through its mapped address; else it must be device memory
        std::lock_guard<std::mutex> lock(g_host_mutex);
        auto it = g_host_allocs.find(const_cast<void *>(rgb));
        if (it != g_host_allocs.end()) {
            if (it->second.bytes < in_bytes) return tr::fail(TR_E_INVALID, "tr_scene_to_yuv_from: the host buffer `rgb` is smaller than the image");
            source = it->second.device;
        }
    }
    if (!source) {
        const char *text = "tr_scene_to_yuv_from: `rgb` is neither device memory nor from tr_host_alloc (tr_yuv_host takes any host memory)";
        hipPointerAttribute_t attr = {};
        if (hipPointerGetAttributes(&attr, rgb) != hipSuccess) {
            (void)hipGetLastError();  // (ordinary host memory is an error to the runtime: not a sticky one)
            return tr::fail(TR_E_INVALID, text);
        }
        if (attr.type != hipMemoryTypeDevice) return tr::fail(TR_E_INVALID, text);
        source = rgb;
    }
    void *target = nullptr;
    st = classify_out(out, bytes, "tr_scene_to_yuv_from", "tr_yuv_host", "planes", &target);
    if (st != TR_OK) return st;
    if ((const uint8_t *)target < (const uint8_t *)source + in_bytes && (const uint8_t *)source < (const uint8_t *)target + bytes)
        return tr::fail(TR_E_INVALID, "tr_scene_to_yuv_from: `rgb` overlaps `out` (there is no in-place form)");
    // behind everything issued so far, held-back frames included: the image may be a stage's output of this scene
    if ((st = submit_pending(s)) != TR_OK) return st;
    return launch_yuv_on(s, (const uint8_t *)source, nullptr, width, height, p, (uint8_t *)target);
}

int tr_scene_get_yuv(tr_scene *s, const tr_yuv_params *p, uint8_t *planes)
{
    if (!s) return tr::fail(TR_E_INVALID, "tr_scene_get_yuv: null scene");
    if (!planes) return tr::fail(TR_E_INVALID, "tr_scene_get_yuv: null argument");
    int st = check_yuv_params(p, "tr_scene_get_yuv");
    if (st == TR_OK) st = check_yuv_size(s->width, s->height, "tr_scene_get_yuv");
    if (st == TR_OK) st = check_yuv_scene(s, "tr_scene_get_yuv");
    if (st != TR_OK) return st;
    // (no short circuit: a cleared scene's planes are not zeros; enqueue_yuv fills them)
    return get_stage(s, planes, yuv_bytes(s->width, s->height, p->layout), nullptr, [&](uint8_t *o) { return enqueue_yuv(s, p, o); });
}

// The rule of tr_yuv.h over a caller's array, on the host.  Needs no GPU.
int tr_yuv_host(uint32_t width, uint32_t height, const uint8_t *rgb, const tr_yuv_params *p, uint8_t *out)
{
    int st = check_yuv_params(p, "tr_yuv_host");
    if (st == TR_OK) st = check_yuv_size(width, height, "tr_yuv_host");
    if (st != TR_OK) return st;
    if (!rgb || !out) return tr::fail(TR_E_INVALID, "tr_yuv_host: null argument");
    if (out == rgb) return tr::fail(TR_E_INVALID, "tr_yuv_host: out is rgb (the sizes differ: not in place)");
    yuv_host(width, height, rgb, yuv_rule(p), out);
    return TR_OK;
}

size_t tr_yuv_bytes(uint32_t width, uint32_t height, uint32_t layout)
{
    if (!yuv_layout_ok(layout) || width < 1u || width > YUV_MAX_SIDE || height < 1u || height > YUV_MAX_SIDE) {
        (void)tr::fail(TR_E_INVALID, "tr_yuv_bytes: an unknown layout, or width and height not 1..8192");
        return 0u;
    }
    return yuv_bytes(width, height, layout);
}

int tr_yuv_plane(uint32_t width, uint32_t height, uint32_t layout, uint32_t plane, size_t *offset, uint32_t *w, uint32_t *h, uint32_t *step)
{
    if (!offset || !w || !h || !step) return tr::fail(TR_E_INVALID, "tr_yuv_plane: null argument");
    if (!yuv_layout_ok(layout)) return tr::fail(TR_E_INVALID, "tr_yuv_plane: layout must be TR_YUV_I420, TR_YUV_NV12 or TR_YUV_I444");
    int st = check_yuv_size(width, height, "tr_yuv_plane");
    if (st != TR_OK) return st;
    if (!yuv_plane(width, height, layout, plane, offset, w, h, step)) return tr::fail(TR_E_INVALID, "tr_yuv_plane: the layout has no such plane");
    return TR_OK;
}

int tr_yuv_coefficients(uint32_t matrix, uint32_t range, int32_t *out10)
{
    if (!out10) return tr::fail(TR_E_INVALID, "tr_yuv_coefficients: null argument");
    if (matrix > TR_YUV_BT709 || range > TR_YUV_LIMITED) return tr::fail(TR_E_INVALID, "tr_yuv_coefficients: an unknown matrix or range");
    const YuvRule &k = kYuvTables[matrix][range];
    for (int c = 0; c < 3; c++) out10[c] = k.y[c], out10[3 + c] = k.u[c], out10[6 + c] = k.v[c];
    out10[9] = k.y0;
    return TR_OK;
}

namespace {

static_assert(TR_LAYER_NORMAL == LAYER_NORMAL && TR_LAYER_ADD == LAYER_ADD && TR_LAYER_MULTIPLY == LAYER_MULTIPLY && TR_LAYER_SCREEN == LAYER_SCREEN &&
                  TR_LAYER_LIGHTEN == LAYER_LIGHTEN && TR_LAYER_DARKEN == LAYER_DARKEN && TR_LAYER_DIFFERENCE == LAYER_DIFFERENCE &&
                  TR_LAYER_RGB8 == LAYER_RGB8 && TR_LAYER_RGBA8 == LAYER_RGBA8 && TR_LAYER_KEY == LAYER_KEY && TR_LAYER_WHERE_DRAWN == LAYER_WHERE_DRAWN &&
                  TR_LAYER_WHERE_UNDRAWN == LAYER_WHERE_UNDRAWN && TR_LAYER_MAX_SIDE == LAYER_MAX_SIDE && sizeof(tr_layer_params) == 40,
              "tr_layer.h restates the header");

constexpr uint32_t kLayerWhere = TR_LAYER_WHERE_DRAWN | TR_LAYER_WHERE_UNDRAWN;

// tr_layer_params as every entry point accepts them (`who` names the entry point in the error text).  from_scene: the
// layer is another scene's frame, and its size and stride are that scene's.
int check_layer_params(const tr_layer_params *p, bool from_scene, const char *who)
{
    const std::string w(who);
    if (!p) return tr::fail(TR_E_INVALID, w + ": null argument");
    if (p->mode > TR_LAYER_DIFFERENCE) return tr::fail(TR_E_INVALID, w + ": mode must be TR_LAYER_NORMAL .. TR_LAYER_DIFFERENCE");
    if (p->format != TR_LAYER_RGB8 && p->format != TR_LAYER_RGBA8) return tr::fail(TR_E_INVALID, w + ": format must be TR_LAYER_RGB8 or TR_LAYER_RGBA8");
    if ((p->flags & ~(TR_LAYER_KEY | kLayerWhere)) != 0u) return tr::fail(TR_E_INVALID, w + ": unknown flags");
    if ((p->flags & kLayerWhere) == kLayerWhere)
        return tr::fail(TR_E_INVALID, w + ": TR_LAYER_WHERE_DRAWN and TR_LAYER_WHERE_UNDRAWN exclude each other");
    if (p->opacity > 256u) return tr::fail(TR_E_INVALID, w + ": opacity must be 0..256");
    if (from_scene) {
        if (p->format != TR_LAYER_RGB8) return tr::fail(TR_E_INVALID, w + ": format must be TR_LAYER_RGB8 (a scene's frame is rgb8)");
        if (p->width != 0u || p->height != 0u || p->stride != 0u)
            return tr::fail(TR_E_INVALID, w + ": width, height and stride must be 0 (they are taken from src)");
        return TR_OK;
    }
    if (p->width < 1u || p->width > LAYER_MAX_SIDE || p->height < 1u || p->height > LAYER_MAX_SIDE)
        return tr::fail(TR_E_INVALID, w + ": width and height must be 1..8192");
    if (p->stride != 0u && p->stride < p->width * layer_bpp(p->format))
        return tr::fail(TR_E_INVALID, w + ": stride must be 0 or at least the bytes of a row");
    return TR_OK;
}

int check_layer_scene(const tr_scene *s, const char *who)
{
    if (!whole_frame(s))
        return tr::fail(TR_E_INVALID, std::string(who) + ": a band scene (tr_options.band_row0/1) cannot be layered: "
                                                         "the layer's rows would have to be split among the ranks");
    if (s->broken) return unusable();
    return TR_OK;
}

// The rule of checked parameters for a layer of width x height pixels.
LayerRule layer_rule(const tr_layer_params *p, uint32_t width, uint32_t height)
{
    LayerRule r;
    r.mode = p->mode, r.format = p->format, r.flags = p->flags, r.opacity = p->opacity;
    r.x = p->x, r.y = p->y;
    r.width = width, r.height = height;
    r.stride = p->stride ? p->stride : width * layer_bpp(p->format);
    r.key = grade_pack(p->key[0], p->key[1], p->key[2]);
    return r;
}

// Does the layer's rectangle miss a W x H frame (or cover nothing: opacity 0)?
bool layer_misses(const LayerRule &r, uint32_t W, uint32_t H)
{
    return r.opacity == 0u || r.x >= (int64_t)W || r.y >= (int64_t)H || (int64_t)r.x + r.width <= 0 || (int64_t)r.y + r.height <= 0;
}

// `image` of a layer (or a projector: what / host_rule are the error texts' words): memory from tr_host_alloc of at least
// `bytes` bytes (its mapped address) or device memory.
int classify_layer_image(const void *image, size_t bytes, const char *who, const void **source_out, const char *what = "layer",
                         const char *host_rule = "tr_layer_host")
{
    const std::string w(who);
    const void *source = nullptr;
    {
        std::lock_guard<std::mutex> lock(g_host_mutex);
        auto it = g_host_allocs.find(const_cast<void *>(image));
        if (it != g_host_allocs.end()) {
            if (it->second.bytes < bytes) return tr::fail(TR_E_INVALID, w + ": the host buffer `image` is smaller than the " + what);
            source = it->second.device;
        }
    }
    if (!source) {
        const std::string text = w + ": `image` is neither device memory nor from tr_host_alloc (" + host_rule + " takes any host memory)";
        hipPointerAttribute_t attr = {};
        if (hipPointerGetAttributes(&attr, image) != hipSuccess) {
            (void)hipGetLastError();  // (ordinary host memory is an error to the runtime: not a sticky one)
            return tr::fail(TR_E_INVALID, text);
        }
        if (attr.type != hipMemoryTypeDevice) return tr::fail(TR_E_INVALID, text);
        source = image;
    }
    *source_out = source;
    return TR_OK;
}

// Enqueues the blend of the layer `image` (r's; src: the scene whose current frame it is, or null) into `out_device`
// (null: in place) behind everything issued so far.  A pending clear is made real: in place the kernel then runs on the
// raised flags, out of place it writes the layer over zeros.  Depth is needed only with a WHERE flag; without one a
// depth left on the chip stays there.
int enqueue_layer(tr_scene *s, const LayerRule &r, const uint8_t *image, tr_scene *src, uint8_t *out_device)
{
    int st = flush_clear_color(s);  // (submits what is held back, too)
    if (st == TR_OK && (r.flags & kLayerWhere)) st = depth_in_memory(s);
    // src's frame on its way; a logically cleared frame is a layer of zeros whatever its memory holds
    if (st == TR_OK && src) st = submit_pending(src);
    if (st != TR_OK) return st;
    LayerArgs a = {};
    a.fb = s->d_fb;
    a.fbclean = s->d_fbclean;
    a.out = out_device ? out_device : s->d_fb;
    a.lower = out_device ? nullptr : s->d_fbclean;
    if (r.flags & kLayerWhere) a.z = s->d_z, a.zclean = s->d_zclean;
    a.image = image;
    if (src) {
        a.src_clean = src->d_fbclean;
        a.src_ntx = (src->width + (uint32_t)TILE_W - 1u) / (uint32_t)TILE_W;
        a.src_all_clean = src->z_fb_cleared ? 1u : 0u;
    }
    a.frame = s->frame;
    a.rule = r;
    auto launch = [&] {
        Timed t(s, K_LAYER);
        int rc = launch_layer(a, src != nullptr, s->stream);
        return rc ? launch_status(rc, "k_layer") : TR_OK;
    };
    if (src) return cross_scene_launch(s, src, launch);
    if ((st = launch()) != TR_OK) return st;
    s->quiescent = false;
    return TR_OK;
}

// What tr_scene_layer and tr_scene_layer_from_scene share once the layer is known: `out`, the overlaps, the shortcuts.
int layer_into(tr_scene *s, const LayerRule &r, const uint8_t *image, tr_scene *src, void *out, const char *who)
{
    void *target = nullptr;
    int st = frame_out(s, out, who, "tr_scene_get_layered", "layers", 0u, &target);
    if (st != TR_OK) return st;
    const size_t image_bytes = (size_t)layer_block_bytes(r.width, r.height, r.stride, r.format);
    if (target && (const uint8_t *)target < image + image_bytes && image < (const uint8_t *)target + frame_bytes(s))
        return tr::fail(TR_E_INVALID, std::string(who) + (src ? ": `out` overlaps a frame buffer of src" : ": `image` overlaps `out`"));
    if (!src && refuse_overlap(s, image, frame_bytes(s), who, "layers", 0u, image_bytes) != TR_OK)
        return tr::fail(TR_E_INVALID, std::string(who) + ": `image` overlaps a frame buffer of the scene");
    if (target && src && refuse_overlap(src, target, frame_bytes(src), who, "layers", 0u, frame_bytes(s)) != TR_OK)
        return tr::fail(TR_E_INVALID, std::string(who) + ": `out` overlaps a frame buffer of src");
    if (layer_misses(r, s->width, s->height)) {
        // nothing is blended: in place nothing happens, out of place a copy -- of black without a kernel
        if (!target) return TR_OK;
        if (s->z_fb_cleared) return cleared_out_of_place(s, target);
    }
    st = enqueue_layer(s, r, image, src, (uint8_t *)target);
    if (st == TR_OK && !src) handed_on(s);
    return st;
}

}  // namespace

int tr_scene_layer(tr_scene *s, const tr_layer_params *p, const void *image, void *out)
{
    if (!s) return tr::fail(TR_E_INVALID, "tr_scene_layer: null scene");
    int st = check_layer_params(p, false, "tr_scene_layer");
    if (st == TR_OK && !image) st = tr::fail(TR_E_INVALID, "tr_scene_layer: null argument");
    if (st == TR_OK) st = check_layer_scene(s, "tr_scene_layer");
    if (st != TR_OK) return st;
    HIP_TRY(hipSetDevice(s->device));
    const LayerRule r = layer_rule(p, p->width, p->height);
    const void *source = nullptr;
    st = classify_layer_image(image, (size_t)layer_block_bytes(r.width, r.height, r.stride, r.format), "tr_scene_layer", &source);
    if (st != TR_OK) return st;
    return layer_into(s, r, (const uint8_t *)source, nullptr, out, "tr_scene_layer");
}

int tr_scene_layer_from_scene(tr_scene *dst, const tr_layer_params *p, tr_scene *src, void *out)
{
    if (!dst || !src) return tr::fail(TR_E_INVALID, "tr_scene_layer_from_scene: null scene");
    int st = check_layer_params(p, true, "tr_scene_layer_from_scene");
    if (st != TR_OK) return st;
    if (dst == src) return tr::fail(TR_E_INVALID, "tr_scene_layer_from_scene: dst and src are the same scene");
    if (dst->device != src->device) return tr::fail(TR_E_INVALID, "tr_scene_layer_from_scene: the scenes are on different devices");
    if (src->width > LAYER_MAX_SIDE || src->height > LAYER_MAX_SIDE)
        return tr::fail(TR_E_INVALID, "tr_scene_layer_from_scene: src is wider or higher than 8192 (a layer's width and height must be 1..8192)");
    if (!whole_frame(src))
        return tr::fail(TR_E_INVALID, "tr_scene_layer_from_scene: src is a band scene (tr_options.band_row0/1): it holds only its rows of the frame");
    st = check_layer_scene(dst, "tr_scene_layer_from_scene");
    if (st != TR_OK) return st;
    if (src->broken) return unusable();
    HIP_TRY(hipSetDevice(dst->device));
    // what src holds back goes first, as in tr_scene_set_texture_from_frame: its current frame buffer is known after it
    if ((st = submit_pending(src)) != TR_OK) return st;
    return layer_into(dst, layer_rule(p, src->width, src->height), src->d_fb, src, out, "tr_scene_layer_from_scene");
}

int tr_scene_get_layered(tr_scene *s, const tr_layer_params *p, const void *image, uint8_t *rgb)
{
    if (!s) return tr::fail(TR_E_INVALID, "tr_scene_get_layered: null scene");
    int st = check_layer_params(p, false, "tr_scene_get_layered");
    if (st == TR_OK && (!image || !rgb)) st = tr::fail(TR_E_INVALID, "tr_scene_get_layered: null argument");
    if (st == TR_OK) st = check_layer_scene(s, "tr_scene_get_layered");
    if (st != TR_OK) return st;
    HIP_TRY(hipSetDevice(s->device));
    const LayerRule r = layer_rule(p, p->width, p->height);
    const size_t image_bytes = (size_t)layer_block_bytes(r.width, r.height, r.stride, r.format);
    const void *source = nullptr;
    st = classify_layer_image(image, image_bytes, "tr_scene_get_layered", &source);
    if (st != TR_OK) return st;
    if (refuse_overlap(s, source, frame_bytes(s), "tr_scene_get_layered", "layers", 0u, image_bytes) != TR_OK)
        return tr::fail(TR_E_INVALID, "tr_scene_get_layered: `image` overlaps a frame buffer of the scene");
    // (a cleared scene is zeros only where nothing is blended)
    return get_stage(s, rgb, frame_bytes(s), layer_misses(r, s->width, s->height) ? cleared : nullptr,
                     [&](uint8_t *o) { return enqueue_layer(s, r, (const uint8_t *)source, nullptr, o); });
}

// The rule of tr_layer.h over caller's arrays, on the host.  Needs no GPU.
int tr_layer_host(uint32_t width, uint32_t height, const uint8_t *rgb, const float *z, const tr_layer_params *p, const uint8_t *image, uint8_t *out)
{
    int st = check_layer_params(p, false, "tr_layer_host");
    if (st != TR_OK) return st;
    if (width < 1u || height < 1u) return tr::fail(TR_E_INVALID, "tr_layer_host: the frame's width and height must be at least 1");
    if (!rgb || !image || !out) return tr::fail(TR_E_INVALID, "tr_layer_host: null argument");
    if ((p->flags & kLayerWhere) && !z) return tr::fail(TR_E_INVALID, "tr_layer_host: a WHERE flag needs z");
    layer_host(width, height, rgb, z, layer_rule(p, p->width, p->height), image, out);
    return TR_OK;
}

namespace {

static_assert(TR_RAMP_MAX_N == RAMP_MAX_N && TR_RAMP_REPEAT == RAMP_REPEAT && sizeof(tr_ramp_params) == 32, "tr_ramp.h restates the header");

// tr_ramp_params as every entry point accepts them (`who` names the entry point in the error text).
int check_ramp_params(const tr_ramp_params *p, const char *who)
{
    const std::string w(who);
    if (!p) return tr::fail(TR_E_INVALID, w + ": null argument");
    if (!std::isfinite(p->z0)) return tr::fail(TR_E_INVALID, w + ": z0 must be finite");
    if (!std::isfinite(p->scale) || p->scale == 0.0f) return tr::fail(TR_E_INVALID, w + ": scale must be finite and not 0");
    if (p->mode > TR_LAYER_DIFFERENCE) return tr::fail(TR_E_INVALID, w + ": mode must be TR_LAYER_NORMAL .. TR_LAYER_DIFFERENCE");
    if (p->opacity > 256u) return tr::fail(TR_E_INVALID, w + ": opacity must be 0..256");
    if ((p->flags & ~TR_RAMP_REPEAT) != 0u) return tr::fail(TR_E_INVALID, w + ": unknown flags");
    if (p->reserved[0] != 0u || p->reserved[1] != 0u) return tr::fail(TR_E_INVALID, w + ": reserved must be 0");
    return TR_OK;
}

int check_ramp_n(uint32_t n, const char *who)
{
    if (n < 2u || n > RAMP_MAX_N) return tr::fail(TR_E_INVALID, std::string(who) + ": the table's length n must be 2..TR_RAMP_MAX_N");
    return TR_OK;
}

int check_ramp_scene(const tr_scene *s, const char *who)
{
    if (s->ramp_n == 0u) return tr::fail(TR_E_INVALID, std::string(who) + ": the scene has no ramp table (tr_scene_set_ramp)");
    if (!whole_frame(s))
        return tr::fail(TR_E_INVALID, std::string(who) + ": a band scene (tr_options.band_row0/1) cannot be ramped");
    if (s->broken) return unusable();
    return TR_OK;
}

// The rule of checked parameters over a table of n entries.
RampRule ramp_rule(const tr_ramp_params *p, uint32_t n)
{
    RampRule r;
    r.z0 = p->z0, r.scale = p->scale;
    r.mode = p->mode, r.opacity = p->opacity, r.undrawn = p->undrawn, r.flags = p->flags;
    r.n = n;
    return r;
}

// Enqueues the ramp of the current frame into `out_device` (null: in place) behind everything issued so far.  A pending
// clear is made real (the kernel then runs on raised flags), and the stage always reads depth: one left on the chip is
// made real first.
int enqueue_ramp(tr_scene *s, const RampRule &r, uint8_t *out_device)
{
    int st = flush_clear_color(s);  // (submits what is held back, too)
    if (st == TR_OK) st = depth_in_memory(s);
    if (st != TR_OK) return st;
    RampArgs a = {};
    a.fb = s->d_fb;
    a.fbclean = s->d_fbclean;
    a.out = out_device ? out_device : s->d_fb;
    a.lower = out_device ? nullptr : s->d_fbclean;
    a.z = s->d_z;
    a.zclean = s->d_zclean;
    a.table = s->d_ramp;
    a.frame = s->frame;
    a.rule = r;
    return timed_launch(s, K_RAMP, "k_ramp", [&] { return launch_ramp(a, s->stream, s->ramp_cap, &s->ramp_grid); });
}

}  // namespace

int tr_scene_set_ramp(tr_scene *s, uint32_t n, const uint8_t *rgba)
{
    if (!s) return tr::fail(TR_E_INVALID, "tr_scene_set_ramp: null scene");
    if (n != 0u) {
        int st = check_ramp_n(n, "tr_scene_set_ramp");
        if (st != TR_OK) return st;
        if (!rgba) return tr::fail(TR_E_INVALID, "tr_scene_set_ramp: null table");
    }
    HIP_TRY(hipSetDevice(s->device));
    // one word an entry, padded to whole 16-byte pieces (k_ramp stages the table by pieces)
    const size_t padded = ((size_t)n + 3u) / 4u * 4u;
    std::vector<uint32_t> words(padded, 0u);
    if (n) ramp_expand(n, rgba, words.data());
    int st = swap_device_array(s, s->d_ramp, n != 0u, words.data(), padded);
    if (st != TR_OK) return st;
    s->ramp_n = n;
    return TR_OK;
}

int tr_scene_ramp(tr_scene *s, const tr_ramp_params *p, void *out)
{
    if (!s) return tr::fail(TR_E_INVALID, "tr_scene_ramp: null scene");
    int st = check_ramp_params(p, "tr_scene_ramp");
    if (st == TR_OK) st = check_ramp_scene(s, "tr_scene_ramp");
    if (st != TR_OK) return st;
    HIP_TRY(hipSetDevice(s->device));
    void *target = nullptr;
    st = frame_out(s, out, "tr_scene_ramp", "tr_scene_get_ramped", "ramps", 0u, &target);
    if (st != TR_OK) return st;
    const RampRule r = ramp_rule(p, s->ramp_n);
    // a logically cleared scene is `undrawn` over black everywhere: zeros out of place, itself in place
    if (s->z_fb_cleared && ramp_keeps_cleared_black(r)) return target ? cleared_out_of_place(s, target) : TR_OK;
    st = enqueue_ramp(s, r, (uint8_t *)target);
    if (st == TR_OK) handed_on(s);
    return st;
}

int tr_scene_get_ramped(tr_scene *s, const tr_ramp_params *p, uint8_t *rgb)
{
    if (!s) return tr::fail(TR_E_INVALID, "tr_scene_get_ramped: null scene");
    int st = check_ramp_params(p, "tr_scene_get_ramped");
    if (st == TR_OK && !rgb) st = tr::fail(TR_E_INVALID, "tr_scene_get_ramped: null argument");
    if (st == TR_OK) st = check_ramp_scene(s, "tr_scene_get_ramped");
    if (st != TR_OK) return st;
    HIP_TRY(hipSetDevice(s->device));
    const RampRule r = ramp_rule(p, s->ramp_n);
    return get_stage(s, rgb, frame_bytes(s), ramp_keeps_cleared_black(r) ? cleared : nullptr, [&](uint8_t *o) { return enqueue_ramp(s, r, o); });
}

// The rule of tr_ramp.h over caller's arrays, on the host.  Needs no GPU.
int tr_ramp_host(uint32_t width, uint32_t height, const uint8_t *rgb, const float *z, const tr_ramp_params *p, uint32_t n, const uint8_t *table,
                 uint8_t *out)
{
    int st = check_ramp_params(p, "tr_ramp_host");
    if (st == TR_OK) st = check_ramp_n(n, "tr_ramp_host");
    if (st != TR_OK) return st;
    if (width < 1u || height < 1u) return tr::fail(TR_E_INVALID, "tr_ramp_host: the frame's width and height must be at least 1");
    if (!rgb || !z || !table || !out) return tr::fail(TR_E_INVALID, "tr_ramp_host: null argument");
    ramp_host(width, height, rgb, z, ramp_rule(p, n), table, out);
    return TR_OK;
}

int tr_ramp_positions(const tr_ramp_params *p, uint32_t n, uint32_t count, const float *z, uint32_t *positions)
{
    int st = check_ramp_params(p, "tr_ramp_positions");
    if (st == TR_OK) st = check_ramp_n(n, "tr_ramp_positions");
    if (st != TR_OK) return st;
    if (count == 0u) return TR_OK;
    if (!z || !positions) return tr::fail(TR_E_INVALID, "tr_ramp_positions: null argument");
    const RampRule r = ramp_rule(p, n);
    for (uint32_t k = 0; k < count; k++) positions[k] = layer_drawn(z[k]) ? ramp_position(z[k], r) : RAMP_NO_POSITION;
    return TR_OK;
}

int tr_scene_debug_ramp_grid(tr_scene *s, uint32_t cap)
{
    if (!s) return tr::fail(TR_E_INVALID, "tr_scene_debug_ramp_grid: null scene");
    s->ramp_cap = cap;
    return (int)s->ramp_grid;
}

namespace {

static_assert(TR_LINES_MAX_N == LINES_MAX_N && TR_LINES_MAX_WIDTH == LINES_MAX_WIDTH && TR_LINES_DEPTH_TEST == LINES_DEPTH_TEST &&
                  TR_LINES_PAINTER == LINES_PAINTER && sizeof(tr_lines_params) == 32 && sizeof(tr_line) == sizeof(Line) &&
                  offsetof(tr_line, z0) == offsetof(Line, z0) && offsetof(tr_line, x1) == offsetof(Line, x1) && offsetof(tr_line, z1) == offsetof(Line, z1) &&
                  offsetof(tr_line, rgba) == offsetof(Line, rgba) && offsetof(tr_line, reserved) == offsetof(Line, reserved),
              "tr_lines.h restates the header");

// tr_lines_params as every entry point accepts them (`who` names the entry point in the error text).
int check_lines_params(const tr_lines_params *p, const char *who)
{
    const std::string w(who);
    if (!p) return tr::fail(TR_E_INVALID, w + ": null argument");
    if (p->width < 1u || p->width > TR_LINES_MAX_WIDTH) return tr::fail(TR_E_INVALID, w + ": width must be 1..15");
    if (p->opacity > 256u) return tr::fail(TR_E_INVALID, w + ": opacity must be 0..256");
    if ((p->flags & ~(TR_LINES_DEPTH_TEST | TR_LINES_PAINTER)) != 0u) return tr::fail(TR_E_INVALID, w + ": unknown flags");
    if (!std::isfinite(p->depth_bias)) return tr::fail(TR_E_INVALID, w + ": depth_bias must be finite");
    if (p->reserved[0] != 0u || p->reserved[1] != 0u || p->reserved[2] != 0u || p->reserved[3] != 0u) return tr::fail(TR_E_INVALID, w + ": reserved must be 0");
    return TR_OK;
}

// A table of n segments as tr_scene_set_lines and tr_lines_host accept it.
int check_lines_table(uint32_t n, const tr_line *lines, const char *who)
{
    const std::string w(who);
    if (n > LINES_MAX_N) return tr::fail(TR_E_INVALID, w + ": the table's length n must be 0..TR_LINES_MAX_N");
    if (n != 0u && !lines) return tr::fail(TR_E_INVALID, w + ": null table");
    for (uint32_t i = 0; i < n; i++)
        if (const char *why = lines_refusal(reinterpret_cast<const Line *>(lines)[i]))
            return tr::fail(TR_E_INVALID, w + ": segment " + std::to_string(i) + ": " + why);
    return TR_OK;
}

int check_lines_scene(const tr_scene *s, const char *who)
{
    if (s->lines_n == 0u) return tr::fail(TR_E_INVALID, std::string(who) + ": the scene has no table of lines (tr_scene_set_lines)");
    if (!whole_frame(s))
        return tr::fail(TR_E_INVALID, std::string(who) + ": a band scene (tr_options.band_row0/1) cannot take lines: "
                                                         "the table is binned over the whole frame");
    if (s->broken) return unusable();
    return TR_OK;
}

LinesRule lines_rule(const tr_lines_params *p)
{
    LinesRule r;
    r.width = p->width, r.opacity = p->opacity, r.flags = p->flags, r.bias = p->depth_bias;
    return r;
}

// Does nothing reach the frame: a table whose lists are empty, or no coverage?
bool lines_draw_nothing(const tr_scene *s, const LinesRule &r) { return s->lines_entries == 0u || r.opacity == 0u; }

// Enqueues the table drawn over the current frame into `out_device` (null: in place) behind everything issued so far.  A
// pending clear is made real (the kernel then runs on raised flags).  Depth is needed only under the test; without it a
// depth left on the chip stays there.
int enqueue_lines(tr_scene *s, const LinesRule &r, uint8_t *out_device)
{
    int st = flush_clear_color(s);  // (submits what is held back, too)
    if (st == TR_OK && (r.flags & LINES_DEPTH_TEST)) st = depth_in_memory(s);
    if (st != TR_OK) return st;
    LinesArgs a = {};
    a.fb = s->d_fb;
    a.fbclean = s->d_fbclean;
    a.out = out_device ? out_device : s->d_fb;
    a.lower = out_device ? nullptr : s->d_fbclean;
    if (r.flags & LINES_DEPTH_TEST) a.z = s->d_z, a.zclean = s->d_zclean;
    a.lines = reinterpret_cast<const Line *>(s->d_lines);
    a.offsets = s->d_lines + (size_t)s->lines_n * 8u;
    a.tiles = a.offsets + (size_t)s->n_tiles + 1u;
    a.entries = a.tiles + s->lines_listed;
    a.frame = s->frame;
    a.rule = r;
    return timed_launch(s, K_LINES, "k_lines", [&] { return launch_lines(a, s->lines_listed, s->stream); });
}

}  // namespace

int tr_scene_set_lines(tr_scene *s, uint32_t n, const tr_line *lines)
{
    if (!s) return tr::fail(TR_E_INVALID, "tr_scene_set_lines: null scene");
    int st = check_lines_table(n, lines, "tr_scene_set_lines");
    if (st != TR_OK) return st;
    HIP_TRY(hipSetDevice(s->device));
    std::vector<uint32_t> block;
    std::vector<uint32_t> entries, tiles;
    if (n != 0u) {
        std::vector<uint64_t> offsets;
        lines_bin(s->width, s->height, n, reinterpret_cast<const Line *>(lines), offsets, entries, tiles);
        if (offsets.back() > 0xFFFFFFFFull) return tr::fail(TR_E_INVALID, "tr_scene_set_lines: the table's lists hold 2^32 entries or more");
        if (offsets.size() != (size_t)s->n_tiles + 1u) return tr::fail(TR_E_INVALID, "tr_scene_set_lines: a band scene (tr_options.band_row0/1) cannot take lines");
        block.resize((size_t)n * 8u + offsets.size() + tiles.size() + entries.size());
        uint32_t *at = block.data();
        memcpy(at, lines, (size_t)n * 32u), at += (size_t)n * 8u;
        for (uint64_t o : offsets) *at++ = (uint32_t)o;
        if (!tiles.empty()) memcpy(at, tiles.data(), tiles.size() * 4u), at += tiles.size();
        if (!entries.empty()) memcpy(at, entries.data(), entries.size() * 4u);
    }
    st = swap_device_array(s, s->d_lines, n != 0u, block.data(), block.size());
    if (st != TR_OK) return st;
    s->lines_n = n;
    s->lines_listed = (uint32_t)tiles.size();
    s->lines_entries = entries.size();
    return TR_OK;
}

int tr_scene_lines(tr_scene *s, const tr_lines_params *p, void *out)
{
    if (!s) return tr::fail(TR_E_INVALID, "tr_scene_lines: null scene");
    int st = check_lines_params(p, "tr_scene_lines");
    if (st == TR_OK) st = check_lines_scene(s, "tr_scene_lines");
    if (st != TR_OK) return st;
    HIP_TRY(hipSetDevice(s->device));
    void *target = nullptr;
    st = frame_out(s, out, "tr_scene_lines", "tr_scene_get_lined", "draws", 0u, &target);
    if (st != TR_OK) return st;
    const LinesRule r = lines_rule(p);
    if (lines_draw_nothing(s, r)) {
        // nothing is drawn: in place nothing happens, out of place a copy -- of black without a kernel
        if (!target) return TR_OK;
        if (s->z_fb_cleared) return cleared_out_of_place(s, target);
    }
    st = enqueue_lines(s, r, (uint8_t *)target);
    if (st == TR_OK) handed_on(s);
    return st;
}

int tr_scene_get_lined(tr_scene *s, const tr_lines_params *p, uint8_t *rgb)
{
    if (!s) return tr::fail(TR_E_INVALID, "tr_scene_get_lined: null scene");
    int st = check_lines_params(p, "tr_scene_get_lined");
    if (st == TR_OK && !rgb) st = tr::fail(TR_E_INVALID, "tr_scene_get_lined: null argument");
    if (st == TR_OK) st = check_lines_scene(s, "tr_scene_get_lined");
    if (st != TR_OK) return st;
    HIP_TRY(hipSetDevice(s->device));
    const LinesRule r = lines_rule(p);
    // (a cleared scene is zeros only where nothing is drawn)
    return get_stage(s, rgb, frame_bytes(s), lines_draw_nothing(s, r) ? cleared : nullptr, [&](uint8_t *o) { return enqueue_lines(s, r, o); });
}

// The rule of tr_lines.h over caller's arrays, on the host.  Needs no GPU.
int tr_lines_host(uint32_t width, uint32_t height, const uint8_t *rgb, const float *z, const tr_lines_params *p, uint32_t n, const tr_line *lines,
                  uint8_t *out)
{
    int st = check_lines_params(p, "tr_lines_host");
    if (st == TR_OK) st = check_lines_table(n, lines, "tr_lines_host");
    if (st != TR_OK) return st;
    if (width < 1u || height < 1u || width > 32768u || height > 32768u)
        return tr::fail(TR_E_INVALID, "tr_lines_host: the frame's width and height must be 1..32768");
    if (!rgb || !out || ((p->flags & TR_LINES_DEPTH_TEST) && !z)) return tr::fail(TR_E_INVALID, "tr_lines_host: null argument");
    lines_host(width, height, rgb, z, lines_rule(p), n, reinterpret_cast<const Line *>(lines), out);
    return TR_OK;
}

int tr_scene_debug_line_bins(tr_scene *s, uint32_t *n_tiles, uint64_t *n_entries)
{
    if (!s || !n_tiles || !n_entries) return tr::fail(TR_E_INVALID, "tr_scene_debug_line_bins: null argument");
    *n_tiles = s->lines_listed;
    *n_entries = s->lines_entries;
    return TR_OK;
}

namespace {

static_assert(TR_DIST_SEED_DRAWN == DIST_SEED_DRAWN && TR_DIST_SEED_KEY == DIST_SEED_KEY && TR_DIST_INVERT == DIST_INVERT && TR_DIST_REPEAT == DIST_REPEAT &&
                  TR_DIST_KEEP_SEEDS == DIST_KEEP_SEEDS && TR_DIST_MAX_RADIUS == DIST_MAX_RADIUS && TR_DIST_FAR == DIST_FAR &&
                  sizeof(tr_distance_params) == 32 && sizeof(tr_distance_ramp_params) == 64,
              "tr_distance.h restates the header");

// tr_distance_params as every entry point accepts them (`who` names the entry point in the error text).
int check_distance_params(const tr_distance_params *p, const char *who)
{
    const std::string w(who);
    if (!p) return tr::fail(TR_E_INVALID, w + ": null argument");
    if (p->seed > TR_DIST_SEED_KEY) return tr::fail(TR_E_INVALID, w + ": seed must be TR_DIST_SEED_DRAWN or TR_DIST_SEED_KEY");
    if (p->threshold > 255u) return tr::fail(TR_E_INVALID, w + ": threshold must be 0..255");
    if (p->radius < 1u || p->radius > TR_DIST_MAX_RADIUS) return tr::fail(TR_E_INVALID, w + ": radius must be 1..TR_DIST_MAX_RADIUS");
    if ((p->flags & ~TR_DIST_INVERT) != 0u) return tr::fail(TR_E_INVALID, w + ": unknown flags");
    for (uint32_t v : p->reserved)
        if (v != 0u) return tr::fail(TR_E_INVALID, w + ": reserved must be 0");
    return TR_OK;
}

int check_distance_ramp_params(const tr_distance_ramp_params *p, const char *who)
{
    const std::string w(who);
    if (!p) return tr::fail(TR_E_INVALID, w + ": null argument");
    int st = check_distance_params(&p->field, who);
    if (st != TR_OK) return st;
    if (p->step < 1u || p->step > DIST_MAX_STEP) return tr::fail(TR_E_INVALID, w + ": step must be 1..65536");
    if (p->mode > TR_LAYER_DIFFERENCE) return tr::fail(TR_E_INVALID, w + ": mode must be TR_LAYER_NORMAL .. TR_LAYER_DIFFERENCE");
    if (p->opacity > 256u) return tr::fail(TR_E_INVALID, w + ": opacity must be 0..256");
    if ((p->flags & ~(TR_DIST_REPEAT | TR_DIST_KEEP_SEEDS)) != 0u) return tr::fail(TR_E_INVALID, w + ": unknown flags");
    for (uint32_t v : p->reserved)
        if (v != 0u) return tr::fail(TR_E_INVALID, w + ": reserved must be 0");
    return TR_OK;
}

int check_distance_scene(const tr_scene *s, bool ramp, const char *who)
{
    if (ramp && s->ramp_n == 0u) return tr::fail(TR_E_INVALID, std::string(who) + ": the scene has no ramp table (tr_scene_set_ramp)");
    if (!whole_frame(s))
        return tr::fail(TR_E_INVALID, std::string(who) + ": a band scene (tr_options.band_row0/1) has no distance field");
    if (s->broken) return unusable();
    return TR_OK;
}

int check_distance_size(uint32_t width, uint32_t height, const char *who)
{
    if (width < 1u || height < 1u || width > 32768u || height > 32768u)
        return tr::fail(TR_E_INVALID, std::string(who) + ": the frame's width and height must be 1..32768");
    return TR_OK;
}

DistRule distance_rule(const tr_distance_params *p)
{
    DistRule r;
    r.seed = p->seed, r.threshold = p->threshold, r.radius = p->radius, r.flags = p->flags;
    return r;
}

DistRampRule distance_ramp_rule(const tr_distance_ramp_params *p, uint32_t n)
{
    DistRampRule r;
    r.field = distance_rule(&p->field);
    r.step = p->step, r.mode = p->mode, r.opacity = p->opacity, r.far = p->far, r.flags = p->flags;
    r.n = n;
    return r;
}

size_t field_bytes(const tr_scene *s) { return (size_t)s->width * s->height * 2; }

// Enqueues the field of the current frame into `field_device` behind everything issued so far: a pending clear is made
// real (the mask kernel then runs on raised flags); under DRAWN a depth left on the chip is made real, under KEY it
// stays where it is.  The scratch is allocated on first use and kept.
int enqueue_distance(tr_scene *s, const DistRule &r, uint16_t *field_device)
{
    int st = flush_clear_color(s);  // (submits what is held back, too)
    if (st == TR_OK && r.seed == DIST_SEED_DRAWN) st = depth_in_memory(s);
    if (st != TR_OK) return st;
    const size_t words = (size_t)dist_words_per_row(s->width) * s->height;
    if (!s->d_dist_mask && (st = dev_alloc(&s->d_dist_mask, words))) return st;
    if (!s->d_dist_h && (st = dev_alloc(&s->d_dist_h, (size_t)s->width * s->height))) return st;
    if (!s->d_dist_summary && (st = dev_alloc(&s->d_dist_summary, words))) return st;
    DistArgs a = {};
    a.fb = s->d_fb;
    a.fbclean = s->d_fbclean;
    a.z = r.seed == DIST_SEED_DRAWN ? s->d_z : nullptr;
    a.zclean = r.seed == DIST_SEED_DRAWN ? s->d_zclean : nullptr;
    a.mask = s->d_dist_mask;
    a.h = s->d_dist_h;
    a.summary = s->d_dist_summary;
    a.field = field_device;
    a.frame = s->frame;
    a.rule = r;
    // (the profile has one name for the three: a call shows 3 launches of "k_dist" and their summed time -- the table of
    // names is as long as tr_scene_profile_read's callers expect it at most)
    st = timed_launch(s, K_DIST, "k_dist_mask", [&] { return launch_dist_mask(a, s->stream); });
    if (st == TR_OK) st = timed_launch(s, K_DIST, "k_dist_row", [&] { return launch_dist_row(a, s->stream); });
    if (st == TR_OK) st = timed_launch(s, K_DIST, "k_dist", [&] { return launch_dist(a, s->stream); });
    return st;
}

// Enqueues the distance ramp of the current frame into `out_device` (null: in place): the field into the scene's
// scratch, then, in stream order, the pointwise kernel.
int enqueue_distance_ramp(tr_scene *s, const DistRampRule &r, uint8_t *out_device)
{
    int st = TR_OK;
    if (!s->d_dist_field && (st = dev_alloc(&s->d_dist_field, (size_t)s->width * s->height))) return st;
    if ((st = enqueue_distance(s, r.field, s->d_dist_field)) != TR_OK) return st;
    DistApplyArgs a = {};
    a.fb = s->d_fb;
    a.fbclean = s->d_fbclean;
    a.out = out_device ? out_device : s->d_fb;
    a.lower = out_device ? nullptr : s->d_fbclean;
    a.field = s->d_dist_field;
    a.table = s->d_ramp;
    a.frame = s->frame;
    a.rule = r;
    return timed_launch(s, K_DIST_APPLY, "k_dist_apply", [&] { return launch_dist_apply(a, s->stream); });
}

}  // namespace

int tr_scene_distance(tr_scene *s, const tr_distance_params *p, void *out)
{
    if (!s) return tr::fail(TR_E_INVALID, "tr_scene_distance: null scene");
    int st = check_distance_params(p, "tr_scene_distance");
    if (st == TR_OK) st = check_distance_scene(s, false, "tr_scene_distance");
    if (st != TR_OK) return st;
    if (!out) return tr::fail(TR_E_INVALID, "tr_scene_distance: out == NULL (the field is no frame of the scene: there is no in-place form)");
    HIP_TRY(hipSetDevice(s->device));
    void *target = nullptr;
    st = classify_out(out, field_bytes(s), "tr_scene_distance", "tr_scene_get_distance", "field", &target);
    if (st != TR_OK) return st;
    if ((uintptr_t)target % 2u != 0u) return tr::fail(TR_E_INVALID, "tr_scene_distance: `out` must be 2-byte aligned");
    if (refuse_overlap(s, target, frame_bytes(s), "tr_scene_distance", "computes", 0u, field_bytes(s)) != TR_OK)
        return tr::fail(TR_E_INVALID, "tr_scene_distance: `out` overlaps a frame buffer of the scene (there is no in-place form)");
    if ((st = enqueue_distance(s, distance_rule(p), (uint16_t *)target)) != TR_OK) return st;
    handed_on(s);
    return TR_OK;
}

int tr_scene_get_distance(tr_scene *s, const tr_distance_params *p, uint16_t *host)
{
    if (!s) return tr::fail(TR_E_INVALID, "tr_scene_get_distance: null scene");
    int st = check_distance_params(p, "tr_scene_get_distance");
    if (st == TR_OK && !host) st = tr::fail(TR_E_INVALID, "tr_scene_get_distance: null argument");
    if (st == TR_OK) st = check_distance_scene(s, false, "tr_scene_get_distance");
    if (st != TR_OK) return st;
    HIP_TRY(hipSetDevice(s->device));
    const DistRule r = distance_rule(p);
    return get_stage(s, (uint8_t *)host, field_bytes(s), nullptr, [&](uint8_t *o) { return enqueue_distance(s, r, (uint16_t *)o); });
}

int tr_scene_distance_ramp(tr_scene *s, const tr_distance_ramp_params *p, void *out)
{
    if (!s) return tr::fail(TR_E_INVALID, "tr_scene_distance_ramp: null scene");
    int st = check_distance_ramp_params(p, "tr_scene_distance_ramp");
    if (st == TR_OK) st = check_distance_scene(s, true, "tr_scene_distance_ramp");
    if (st != TR_OK) return st;
    HIP_TRY(hipSetDevice(s->device));
    void *target = nullptr;
    st = frame_out(s, out, "tr_scene_distance_ramp", "tr_scene_get_distance_ramped", "ramps", 0u, &target);
    if (st != TR_OK) return st;
    st = enqueue_distance_ramp(s, distance_ramp_rule(p, s->ramp_n), (uint8_t *)target);
    if (st == TR_OK) handed_on(s);
    return st;
}

int tr_scene_get_distance_ramped(tr_scene *s, const tr_distance_ramp_params *p, uint8_t *rgb)
{
    if (!s) return tr::fail(TR_E_INVALID, "tr_scene_get_distance_ramped: null scene");
    int st = check_distance_ramp_params(p, "tr_scene_get_distance_ramped");
    if (st == TR_OK && !rgb) st = tr::fail(TR_E_INVALID, "tr_scene_get_distance_ramped: null argument");
    if (st == TR_OK) st = check_distance_scene(s, true, "tr_scene_get_distance_ramped");
    if (st != TR_OK) return st;
    HIP_TRY(hipSetDevice(s->device));
    const DistRampRule r = distance_ramp_rule(p, s->ramp_n);
    return get_stage(s, rgb, frame_bytes(s), nullptr, [&](uint8_t *o) { return enqueue_distance_ramp(s, r, o); });
}

// The rules of tr_distance.h over caller's arrays, on the host.  Need no GPU.
int tr_distance_host(uint32_t width, uint32_t height, const uint8_t *rgb, const float *z, const tr_distance_params *p, uint16_t *out_u16)
{
    int st = check_distance_params(p, "tr_distance_host");
    if (st == TR_OK) st = check_distance_size(width, height, "tr_distance_host");
    if (st != TR_OK) return st;
    if (!rgb || !out_u16 || (p->seed == TR_DIST_SEED_DRAWN && !z)) return tr::fail(TR_E_INVALID, "tr_distance_host: null argument");
    distance_host(width, height, rgb, z, distance_rule(p), out_u16);
    return TR_OK;
}

int tr_distance_ramp_host(uint32_t width, uint32_t height, const uint8_t *rgb, const float *z, const tr_distance_ramp_params *p, uint32_t n,
                          const uint8_t *table, uint8_t *out)
{
    int st = check_distance_ramp_params(p, "tr_distance_ramp_host");
    if (st == TR_OK) st = check_ramp_n(n, "tr_distance_ramp_host");
    if (st == TR_OK) st = check_distance_size(width, height, "tr_distance_ramp_host");
    if (st != TR_OK) return st;
    if (!rgb || !table || !out || (p->field.seed == TR_DIST_SEED_DRAWN && !z)) return tr::fail(TR_E_INVALID, "tr_distance_ramp_host: null argument");
    distance_ramp_host(width, height, rgb, z, distance_ramp_rule(p, n), table, out);
    return TR_OK;
}

int tr_distance_positions(uint32_t step, uint32_t count, const uint16_t *d2, uint32_t *dq, uint32_t *positions)
{
    if (step < 1u || step > DIST_MAX_STEP) return tr::fail(TR_E_INVALID, "tr_distance_positions: step must be 1..65536");
    if (count == 0u) return TR_OK;
    if (!d2) return tr::fail(TR_E_INVALID, "tr_distance_positions: null argument");
    for (uint32_t k = 0; k < count; k++)
        if (d2[k] > DIST_MAX_RADIUS * DIST_MAX_RADIUS) return tr::fail(TR_E_INVALID, "tr_distance_positions: a field value above 65025 has no position");
    for (uint32_t k = 0; k < count; k++) {
        if (dq) dq[k] = dist_dq(d2[k]);
        if (positions) positions[k] = dist_position_raw(d2[k], step);
    }
    return TR_OK;
}

// A model-space point as the draw chain's vertex transform places it (project_vertex, tr_shaders.h).  Needs no GPU.
int tr_project_points(const tr_uniforms *u, uint32_t n, const float *xyz, int32_t *xy, float *z, uint8_t *ok)
{
    if (!u) return tr::fail(TR_E_INVALID, "tr_project_points: null argument");
    if (n == 0u) return TR_OK;
    if (!xyz || !xy || !z || !ok) return tr::fail(TR_E_INVALID, "tr_project_points: null argument");
    for (uint32_t k = 0; k < n; k++) {
        int32_t px = 0, py = 0;
        float pz = 0.0f;
        bool good = project_vertex(u->vpmv, make3(xyz[3 * k], xyz[3 * k + 1], xyz[3 * k + 2]), px, py, pz);
        good = good && px >= -LINES_COORD_MAX && px <= LINES_COORD_MAX && py >= -LINES_COORD_MAX && py <= LINES_COORD_MAX && fabsf(pz) <= TR_LINES_Z_MAX;
        xy[2 * k] = good ? px : 0, xy[2 * k + 1] = good ? py : 0;
        z[k] = good ? pz : 0.0f;
        ok[k] = good ? 1u : 0u;
    }
    return TR_OK;
}

namespace {

static_assert(TR_PROJECTOR_OCCLUDE == PROJECTOR_OCCLUDE && TR_PROJECTOR_SOFT == PROJECTOR_SOFT && TR_PROJECTOR_MAX_SIDE == PROJECTOR_MAX_SIDE &&
                  sizeof(tr_projector_params) == 128,
              "tr_projector.h restates the header");

// tr_projector_params and the image's stride as every entry point accepts them (`who` names the entry point in the error
// text).
int check_projector_params(const tr_projector_params *p, const void *image, uint32_t stride, const char *who)
{
    const std::string w(who);
    if (!p || !image) return tr::fail(TR_E_INVALID, w + ": null argument");
    if (p->pw < 1u || p->pw > PROJECTOR_MAX_SIDE || p->ph < 1u || p->ph > PROJECTOR_MAX_SIDE) return tr::fail(TR_E_INVALID, w + ": pw and ph must be 1..8192");
    if (p->channels != 3u && p->channels != 4u) return tr::fail(TR_E_INVALID, w + ": channels must be 3 or 4");
    if (stride < p->pw * p->channels) return tr::fail(TR_E_INVALID, w + ": image_stride must be at least the bytes of a row");
    if (p->mode > TR_LAYER_DIFFERENCE) return tr::fail(TR_E_INVALID, w + ": mode must be TR_LAYER_NORMAL .. TR_LAYER_DIFFERENCE");
    if ((p->flags & ~(TR_PROJECTOR_OCCLUDE | TR_PROJECTOR_SOFT)) != 0u) return tr::fail(TR_E_INVALID, w + ": unknown flags");
    if ((p->flags & TR_PROJECTOR_SOFT) && !(p->flags & TR_PROJECTOR_OCCLUDE))
        return tr::fail(TR_E_INVALID, w + ": TR_PROJECTOR_SOFT needs TR_PROJECTOR_OCCLUDE");
    if (p->opacity > 256u) return tr::fail(TR_E_INVALID, w + ": opacity must be 0..256");
    if (!std::isfinite(p->depth_bias)) return tr::fail(TR_E_INVALID, w + ": depth_bias must be finite");
    for (int i = 0; i < 16; i++)
        if (!std::isfinite(p->m[i])) return tr::fail(TR_E_INVALID, w + ": every entry of m must be finite");
    for (uint32_t v : p->reserved)
        if (v != 0u) return tr::fail(TR_E_INVALID, w + ": reserved must be 0");
    return TR_OK;
}

// The flag and the occluder go together (the scene of the device entry points, the depth array of the host's).
int check_projector_occluder(const tr_projector_params *p, bool have, const char *who)
{
    if ((p->flags & TR_PROJECTOR_OCCLUDE) && !have) return tr::fail(TR_E_INVALID, std::string(who) + ": TR_PROJECTOR_OCCLUDE needs an occluder");
    if (!(p->flags & TR_PROJECTOR_OCCLUDE) && have) return tr::fail(TR_E_INVALID, std::string(who) + ": an occluder needs TR_PROJECTOR_OCCLUDE");
    return TR_OK;
}

int check_projector_scenes(const tr_scene *s, const tr_projector_params *p, const tr_scene *occ, const char *who)
{
    const std::string w(who);
    int st = check_projector_occluder(p, occ != nullptr, who);
    if (st != TR_OK) return st;
    if (!whole_frame(s)) return tr::fail(TR_E_INVALID, w + ": a band scene (tr_options.band_row0/1) cannot be projected on");
    if (occ) {
        if (occ->device != s->device) return tr::fail(TR_E_INVALID, w + ": the scenes are on different devices");
        if (occ->width != p->pw || occ->height != p->ph) return tr::fail(TR_E_INVALID, w + ": the occluder scene's frame is not pw x ph");
        if (!whole_frame(occ))
            return tr::fail(TR_E_INVALID, w + ": the occluder is a band scene (tr_options.band_row0/1): it holds only its rows of the depth");
    }
    if (s->broken || (occ && occ->broken)) return unusable();
    return TR_OK;
}

// The rule of checked parameters.
ProjectorRule projector_rule(const tr_projector_params *p, uint32_t stride)
{
    ProjectorRule r;
    memcpy(r.m, p->m, sizeof r.m);
    r.pw = p->pw, r.ph = p->ph, r.bpp = p->channels, r.mode = p->mode, r.opacity = p->opacity, r.flags = p->flags, r.stride = stride;
    r.depth_bias = p->depth_bias;
    return r;
}

// Enqueues the projection onto the current frame into `out_device` (null: in place) behind everything issued so far.  A
// pending clear is made real (the kernel then runs on raised flags), and the stage always reads depth: one left on the
// chip is made real first.  occ (null without OCCLUDE): its frame goes on its way and its depth is made real too; the
// kernel checks its z flags per texel, nothing is materialised.  A logically cleared occluder shadows nothing: the call
// goes on without the flag and reads nothing of it.
int enqueue_projector(tr_scene *s, const ProjectorRule &r, const uint8_t *image, tr_scene *occ, uint8_t *out_device)
{
    int st = flush_clear_color(s);  // (submits what is held back, too)
    if (st == TR_OK) st = depth_in_memory(s);
    if (st == TR_OK && occ && occ != s) st = submit_pending(occ);
    if (st != TR_OK) return st;
    ProjectorRule q = r;
    if (occ && occ->z_fb_cleared) q.flags = 0u, occ = nullptr;
    if (occ && occ != s && (st = depth_in_memory(occ)) != TR_OK) return st;
    ProjectorArgs a = {};
    a.fb = s->d_fb;
    a.fbclean = s->d_fbclean;
    a.out = out_device ? out_device : s->d_fb;
    a.lower = out_device ? nullptr : s->d_fbclean;
    a.z = s->d_z;
    a.zclean = s->d_zclean;
    a.image = image;
    if (occ) {
        a.occ_z = occ->d_z;
        a.occ_zclean = occ->d_zclean;
        a.occ_ntx = (occ->width + (uint32_t)TILE_W - 1u) / (uint32_t)TILE_W;
    }
    a.frame = s->frame;
    a.rule = q;
    // (no profile entry: the table of names is as long as tr_scene_profile_read's callers expect it at most -- the launches
    // are counted for tr_scene_debug_projector_launches, and scripts/probe_projector.py times the kernel with events)
    auto launch = [&] {
        int rc = launch_projector(a, s->stream);
        if (rc) return launch_status(rc, "k_projector");
        s->projector_launches += 1u;
        s->quiescent = false;
        return (int)TR_OK;
    };
    if (occ && occ != s) return cross_scene_launch(s, occ, launch);
    return launch();
}

// What both device entry points check of the image: where it lives, and that it is apart from the scene's frame buffers.
int projector_image(const tr_scene *s, const ProjectorRule &r, const void *image, const char *who, const void **source)
{
    const size_t image_bytes = (size_t)projector_image_bytes(r);
    int st = classify_layer_image(image, image_bytes, who, source, "image", "tr_projector_host");
    if (st != TR_OK) return st;
    if (refuse_overlap(s, *source, frame_bytes(s), who, "projects", 0u, image_bytes) != TR_OK)
        return tr::fail(TR_E_INVALID, std::string(who) + ": `image` overlaps a frame buffer of the scene");
    return TR_OK;
}

}  // namespace

int tr_scene_projector(tr_scene *s, const tr_projector_params *p, const void *image, uint32_t image_stride, tr_scene *occ, void *out)
{
    const char *who = "tr_scene_projector";
    if (!s) return tr::fail(TR_E_INVALID, "tr_scene_projector: null scene");
    int st = check_projector_params(p, image, image_stride, who);
    if (st == TR_OK) st = check_projector_scenes(s, p, occ, who);
    if (st != TR_OK) return st;
    HIP_TRY(hipSetDevice(s->device));
    const ProjectorRule r = projector_rule(p, image_stride);
    const void *source = nullptr;
    if ((st = projector_image(s, r, image, who, &source)) != TR_OK) return st;
    void *target = nullptr;
    st = frame_out(s, out, who, "tr_scene_get_projector", "projects", 0u, &target);
    if (st != TR_OK) return st;
    const uint8_t *img = (const uint8_t *)source;
    if (target && (const uint8_t *)target < img + projector_image_bytes(r) && img < (const uint8_t *)target + frame_bytes(s))
        return tr::fail(TR_E_INVALID, "tr_scene_projector: `image` overlaps `out`");
    if (target && occ && occ != s && refuse_overlap(occ, target, frame_bytes(occ), who, "projects", 0u, frame_bytes(s)) != TR_OK)
        return tr::fail(TR_E_INVALID, "tr_scene_projector: `out` overlaps a frame buffer of the occluder scene");
    // a logically cleared scene has nothing drawn: zeros out of place, itself in place; opacity 0 in place changes nothing
    if (s->z_fb_cleared) return target ? cleared_out_of_place(s, target) : TR_OK;
    if (r.opacity == 0u && !target) return TR_OK;
    st = enqueue_projector(s, r, img, occ, (uint8_t *)target);
    if (st == TR_OK) handed_on(s);
    return st;
}

int tr_scene_get_projector(tr_scene *s, const tr_projector_params *p, const void *image, uint32_t image_stride, tr_scene *occ, uint8_t *rgb)
{
    const char *who = "tr_scene_get_projector";
    if (!s) return tr::fail(TR_E_INVALID, "tr_scene_get_projector: null scene");
    int st = check_projector_params(p, image, image_stride, who);
    if (st == TR_OK && !rgb) st = tr::fail(TR_E_INVALID, "tr_scene_get_projector: null argument");
    if (st == TR_OK) st = check_projector_scenes(s, p, occ, who);
    if (st != TR_OK) return st;
    HIP_TRY(hipSetDevice(s->device));
    const ProjectorRule r = projector_rule(p, image_stride);
    const void *source = nullptr;
    if ((st = projector_image(s, r, image, who, &source)) != TR_OK) return st;
    return get_stage(s, rgb, frame_bytes(s), cleared, [&](uint8_t *o) { return enqueue_projector(s, r, (const uint8_t *)source, occ, o); });
}

int tr_scene_debug_projector_launches(tr_scene *s)
{
    if (!s) return tr::fail(TR_E_INVALID, "tr_scene_debug_projector_launches: null scene");
    return (int)s->projector_launches;
}

// The rule of tr_projector.h over caller's arrays, on the host.  Needs no GPU.
int tr_projector_host(uint32_t width, uint32_t height, const uint8_t *rgb, const float *z, const tr_projector_params *p, const void *image,
                      uint32_t image_stride, const float *occluder_z, uint8_t *out)
{
    int st = check_projector_params(p, image, image_stride, "tr_projector_host");
    if (st == TR_OK) st = check_projector_occluder(p, occluder_z != nullptr, "tr_projector_host");
    if (st != TR_OK) return st;
    if (width < 1u || width > 32768u || height < 1u || height > 32768u)
        return tr::fail(TR_E_INVALID, "tr_projector_host: the frame's width and height must be 1..32768");
    if (!rgb || !z || !out) return tr::fail(TR_E_INVALID, "tr_projector_host: null argument");
    projector_host(width, height, rgb, z, projector_rule(p, image_stride), (const uint8_t *)image, occluder_z, out);
    return TR_OK;
}

// projector->vpmv * view->i_vpmv (both column-major), accumulated in double in the order of the header, rounded once.
int tr_projector_matrix(const tr_uniforms *view, const tr_uniforms *projector, float m[16])
{
    if (!view || !projector || !m) return tr::fail(TR_E_INVALID, "tr_projector_matrix: null argument");
    bool inverse = false;
    for (float v : view->i_vpmv) inverse = inverse || v != 0.0f;
    if (!inverse) return tr::fail(TR_E_INVALID, "tr_projector_matrix: view->i_vpmv is all zeros (tr_prepare_uniforms kind 2 fills it)");
    for (int c = 0; c < 4; c++)
        for (int r = 0; r < 4; r++) {
            const double t0 = (double)projector->vpmv[r] * (double)view->i_vpmv[4 * c], t1 = (double)projector->vpmv[4 + r] * (double)view->i_vpmv[4 * c + 1];
            const double t2 = (double)projector->vpmv[8 + r] * (double)view->i_vpmv[4 * c + 2], t3 = (double)projector->vpmv[12 + r] * (double)view->i_vpmv[4 * c + 3];
            const double s0 = t0 + t1;
            const double s1 = s0 + t2;
            m[4 * c + r] = (float)(s1 + t3);
        }
    return TR_OK;
}

namespace {

static_assert(TR_RELIGHT_MAX_LIGHTS == RELIGHT_MAX_LIGHTS && TR_LIGHT_DIRECTIONAL == RELIGHT_DIRECTIONAL && TR_LIGHT_POINT == RELIGHT_POINT &&
                  TR_LIGHT_SPOT == RELIGHT_SPOT && TR_RELIGHT_ALBEDO == RELIGHT_ALBEDO && TR_RELIGHT_SHOW_NORMALS == RELIGHT_SHOW_NORMALS &&
                  sizeof(tr_relight_params) == 128 && sizeof(tr_light) == 64 && sizeof(tr_light) == sizeof(RelightLight) &&
                  offsetof(tr_light, pos) == offsetof(RelightLight, pos) && offsetof(tr_light, dir) == offsetof(RelightLight, dir) &&
                  offsetof(tr_light, colour) == offsetof(RelightLight, colour) && offsetof(tr_light, intensity) == offsetof(RelightLight, intensity) &&
                  offsetof(tr_light, specular) == offsetof(RelightLight, specular) &&
                  offsetof(tr_light, shininess_log2) == offsetof(RelightLight, shininess_log2),
              "tr_relight.h restates the header");

// tr_relight_params and the light table as every entry point accepts them (`who` names the entry point in the error text).
int check_relight_params(const tr_relight_params *p, const tr_light *lights, uint32_t n_lights, const char *who)
{
    const std::string w(who);
    if (!p || (!lights && n_lights > 0u)) return tr::fail(TR_E_INVALID, w + ": null argument");
    if (n_lights > TR_RELIGHT_MAX_LIGHTS) return tr::fail(TR_E_INVALID, w + ": n_lights must be 0..TR_RELIGHT_MAX_LIGHTS");
    if (p->mode > TR_LAYER_DIFFERENCE) return tr::fail(TR_E_INVALID, w + ": mode must be TR_LAYER_NORMAL .. TR_LAYER_DIFFERENCE");
    if ((p->flags & ~(TR_RELIGHT_ALBEDO | TR_RELIGHT_SHOW_NORMALS)) != 0u) return tr::fail(TR_E_INVALID, w + ": unknown flags");
    if (p->opacity > 256u) return tr::fail(TR_E_INVALID, w + ": opacity must be 0..256");
    for (int i = 0; i < 16; i++)
        if (!std::isfinite(p->u[i])) return tr::fail(TR_E_INVALID, w + ": every entry of u must be finite");
    for (int i = 0; i < 3; i++)
        if (!std::isfinite(p->eye[i])) return tr::fail(TR_E_INVALID, w + ": every entry of eye must be finite");
    if (p->ambient[3] != 0u) return tr::fail(TR_E_INVALID, w + ": the fourth byte of ambient must be 0");
    for (uint32_t v : p->reserved)
        if (v != 0u) return tr::fail(TR_E_INVALID, w + ": reserved must be 0");
    for (uint32_t k = 0; k < n_lights; k++) {
        const tr_light &l = lights[k];
        const std::string wl = w + ": light " + std::to_string(k);
        if (l.kind > TR_LIGHT_SPOT) return tr::fail(TR_E_INVALID, wl + ": kind must be TR_LIGHT_DIRECTIONAL .. TR_LIGHT_SPOT");
        const float f[11] = { l.pos[0], l.pos[1], l.pos[2], l.dir[0], l.dir[1], l.dir[2], l.intensity, l.falloff, l.cos_outer, l.cone_scale, l.specular };
        for (float v : f)
            if (!std::isfinite(v)) return tr::fail(TR_E_INVALID, wl + ": every float must be finite");
        if (l.intensity < 0.0f) return tr::fail(TR_E_INVALID, wl + ": intensity must be >= 0");
        if (l.falloff < 0.0f) return tr::fail(TR_E_INVALID, wl + ": falloff must be >= 0");
        if (l.specular < 0.0f) return tr::fail(TR_E_INVALID, wl + ": specular must be >= 0");
        if (l.kind == TR_LIGHT_SPOT && !(l.cone_scale > 0.0f)) return tr::fail(TR_E_INVALID, wl + ": cone_scale must be > 0");
        if (l.shininess_log2 > RELIGHT_MAX_SHININESS_LOG2) return tr::fail(TR_E_INVALID, wl + ": shininess_log2 must be 0..10");
        if (l.colour[3] != 0u) return tr::fail(TR_E_INVALID, wl + ": the fourth byte of colour must be 0");
        if (l.reserved[0] != 0u || l.reserved[1] != 0u) return tr::fail(TR_E_INVALID, wl + ": reserved must be 0");
    }
    return TR_OK;
}

int check_relight_scene(const tr_scene *s, const char *who)
{
    if (!whole_frame(s))
        return tr::fail(TR_E_INVALID, std::string(who) + ": a band scene (tr_options.band_row0/1) cannot be relit: "
                                                         "its border neighbours lie in another rank's rows");
    if (s->broken) return unusable();
    return TR_OK;
}

// The rule of checked parameters.
RelightRule relight_rule(const tr_relight_params *p, const tr_light *lights, uint32_t n_lights)
{
    RelightRule r = {};
    memcpy(r.u, p->u, sizeof r.u);
    memcpy(r.eye, p->eye, sizeof r.eye);
    r.ambient = grade_pack(p->ambient[0], p->ambient[1], p->ambient[2]);
    r.mode = p->mode, r.opacity = p->opacity, r.flags = p->flags, r.n_lights = n_lights;
    if (n_lights > 0u) memcpy(r.lights, lights, (size_t)n_lights * sizeof(tr_light));
    return r;
}

// Enqueues the lights onto the current frame into `out_device` (null: in place) behind everything issued so far.  A
// pending clear is made real (the kernel then runs on raised flags), and the stage always reads depth: one left on the
// chip is made real first.
int enqueue_relight(tr_scene *s, const RelightRule &r, uint8_t *out_device)
{
    int st = flush_clear_color(s);  // (submits what is held back, too)
    if (st == TR_OK) st = depth_in_memory(s);
    if (st != TR_OK) return st;
    RelightArgs a = {};
    a.fb = s->d_fb;
    a.fbclean = s->d_fbclean;
    a.out = out_device ? out_device : s->d_fb;
    a.lower = out_device ? nullptr : s->d_fbclean;
    a.z = s->d_z;
    a.zclean = s->d_zclean;
    a.frame = s->frame;
    a.rule = r;
    // (no profile entry, like k_projector: the launches are counted for tr_scene_debug_relight_launches, and
    // scripts/probe_relight.py times the kernel with events)
    int rc = launch_relight(a, s->stream);
    if (rc) return launch_status(rc, "k_relight");
    s->relight_launches += 1u;
    s->quiescent = false;
    return TR_OK;
}

// opacity == 0 out of place: the frame as it is.  Tiles behind a raised colour flag hold stale memory, so the copy is
// k_layer's, with a layer that misses the frame: it stores zeros for them.  No k_relight runs.
int relight_copy(tr_scene *s, uint8_t *out_device)
{
    LayerRule miss = {};
    miss.mode = LAYER_NORMAL, miss.format = LAYER_RGB8, miss.opacity = 0u;
    miss.x = (int32_t)s->width, miss.y = 0, miss.width = 1u, miss.height = 1u, miss.stride = 3u;
    // The layer lies one column right of the frame, so its clipped rectangle is empty and k_layer loads no byte of it
    // (layer_into's own road for a layer that misses).  launch_layer still wants an image that is not null and does not
    // overlap `out`: the frame itself is one -- frame_out has refused an `out` that overlaps it -- and is device memory
    // of at least the layer's three bytes, should a later k_layer ever look.
    const uint8_t *never_read = s->d_fb;
    return enqueue_layer(s, miss, never_read, nullptr, out_device);
}

}  // namespace

int tr_scene_relight(tr_scene *s, const tr_relight_params *p, const tr_light *lights, uint32_t n_lights, void *out)
{
    const char *who = "tr_scene_relight";
    if (!s) return tr::fail(TR_E_INVALID, "tr_scene_relight: null scene");
    int st = check_relight_params(p, lights, n_lights, who);
    if (st == TR_OK) st = check_relight_scene(s, who);
    if (st != TR_OK) return st;
    HIP_TRY(hipSetDevice(s->device));
    void *target = nullptr;
    st = frame_out(s, out, who, "tr_scene_get_relit", "relights", 0u, &target);
    if (st != TR_OK) return st;
    // a logically cleared scene has nothing drawn: zeros out of place, itself in place; opacity 0 changes nothing
    if (s->z_fb_cleared) return target ? cleared_out_of_place(s, target) : TR_OK;
    if (p->opacity == 0u) {
        if (!target) return TR_OK;
        st = relight_copy(s, (uint8_t *)target);
    } else {
        st = enqueue_relight(s, relight_rule(p, lights, n_lights), (uint8_t *)target);
    }
    if (st == TR_OK) handed_on(s);
    return st;
}

int tr_scene_get_relit(tr_scene *s, const tr_relight_params *p, const tr_light *lights, uint32_t n_lights, uint8_t *rgb)
{
    const char *who = "tr_scene_get_relit";
    if (!s) return tr::fail(TR_E_INVALID, "tr_scene_get_relit: null scene");
    int st = check_relight_params(p, lights, n_lights, who);
    if (st == TR_OK && !rgb) st = tr::fail(TR_E_INVALID, "tr_scene_get_relit: null argument");
    if (st == TR_OK) st = check_relight_scene(s, who);
    if (st != TR_OK) return st;
    HIP_TRY(hipSetDevice(s->device));
    const RelightRule r = relight_rule(p, lights, n_lights);
    return get_stage(s, rgb, frame_bytes(s), cleared, [&](uint8_t *o) { return r.opacity == 0u ? relight_copy(s, o) : enqueue_relight(s, r, o); });
}

int tr_scene_debug_relight_launches(tr_scene *s)
{
    if (!s) return tr::fail(TR_E_INVALID, "tr_scene_debug_relight_launches: null scene");
    return (int)s->relight_launches;
}

// The rule of tr_relight.h over caller's arrays, on the host.  Needs no GPU.
int tr_relight_host(uint32_t width, uint32_t height, const uint8_t *rgb, const float *z, const tr_relight_params *p, const tr_light *lights,
                    uint32_t n_lights, uint8_t *out)
{
    int st = check_relight_params(p, lights, n_lights, "tr_relight_host");
    if (st != TR_OK) return st;
    if (width < 1u || width > 32768u || height < 1u || height > 32768u)
        return tr::fail(TR_E_INVALID, "tr_relight_host: the frame's width and height must be 1..32768");
    if (!rgb || !z || !out) return tr::fail(TR_E_INVALID, "tr_relight_host: null argument");
    relight_host(width, height, rgb, z, relight_rule(p, lights, n_lights), out);
    return TR_OK;
}

int tr_relight_normals_host(uint32_t width, uint32_t height, const float *z, const tr_relight_params *p, float *normals, uint8_t *valid)
{
    int st = check_relight_params(p, nullptr, 0u, "tr_relight_normals_host");
    if (st != TR_OK) return st;
    if (width < 1u || width > 32768u || height < 1u || height > 32768u)
        return tr::fail(TR_E_INVALID, "tr_relight_normals_host: the frame's width and height must be 1..32768");
    if (!z || !normals || !valid) return tr::fail(TR_E_INVALID, "tr_relight_normals_host: null argument");
    relight_normals_host(width, height, z, p->u, p->eye, normals, valid);
    return TR_OK;
}

namespace {

static_assert(TR_STATS_DEPTH == STATS_DEPTH && sizeof(tr_stats_params) == 32 && sizeof(tr_frame_stats) == sizeof(StatsRecord) &&
                  offsetof(tr_frame_stats, zhist) == offsetof(StatsRecord, zhist) && offsetof(tr_frame_stats, n_pixels) == offsetof(StatsRecord, n_pixels) &&
                  offsetof(tr_frame_stats, z_min) == offsetof(StatsRecord, z_min) && offsetof(tr_frame_stats, box_x0) == offsetof(StatsRecord, box_x0) &&
                  offsetof(tr_frame_stats, reserved) == offsetof(StatsRecord, reserved),
              "tr_stats.h restates the header");

// tr_stats_params as every entry point accepts them for a frame of width x height (`who` names the entry point in the
// error text).
int check_stats_params(const tr_stats_params *p, uint32_t width, uint32_t height, const char *who)
{
    const std::string w(who);
    if (!p) return tr::fail(TR_E_INVALID, w + ": null argument");
    if (p->struct_size != sizeof(tr_stats_params)) return tr::fail(TR_E_INVALID, w + ": struct_size is not sizeof(tr_stats_params)");
    if (p->flags & ~TR_STATS_DEPTH) return tr::fail(TR_E_INVALID, w + ": unknown flags");
    if ((p->w == 0u) != (p->h == 0u)) return tr::fail(TR_E_INVALID, w + ": a window has w and h >= 1, or both 0 for the whole frame");
    if (p->w != 0u && ((uint64_t)p->x0 + p->w > width || (uint64_t)p->y0 + p->h > height))
        return tr::fail(TR_E_INVALID, w + ": the window reaches outside the frame");
    if (p->flags & TR_STATS_DEPTH) {
        if (!std::isfinite(p->z_lo)) return tr::fail(TR_E_INVALID, w + ": z_lo must be finite");
        if (!std::isfinite(p->z_scale) || !(p->z_scale > 0.0f)) return tr::fail(TR_E_INVALID, w + ": z_scale must be finite and > 0");
    }
    return TR_OK;
}

StatsRule stats_rule(const tr_stats_params *p, uint32_t width, uint32_t height, int32_t band_y0, int32_t band_y1)
{
    StatsRule r;
    r.win = stats_window(width, height, p->x0, p->y0, p->w, p->h, band_y0, band_y1);
    r.depth = (p->flags & TR_STATS_DEPTH) ? 1u : 0u;
    r.z_lo = r.depth ? p->z_lo : 0.0f;
    r.z_scale = r.depth ? p->z_scale : 1.0f;
    return r;
}

// Enqueues the statistics of the current frame into `out_device` behind everything issued so far.  Nothing of the scene
// is written: a logically cleared scene stays so (the kernel is told, and treats every tile as flagged).  Without
// TR_STATS_DEPTH no depth is read and a depth left on the chip stays there; with it the depth is made real first.
int enqueue_stats(tr_scene *s, const tr_stats_params *p, uint8_t *out_device)
{
    int st = submit_pending(s);
    if (st != TR_OK) return st;
    const bool depth = (p->flags & TR_STATS_DEPTH) != 0u;
    const bool cleared = s->z_fb_cleared;
    if (depth && !cleared && (st = depth_in_memory(s)) != TR_OK) return st;
    if (!s->d_stats_partials) {
        const uint32_t slots = stats_max_grid(s->frame);
        if (slots == 0u) return tr::fail(TR_E_HIP, "tr_scene_frame_stats: the device does not tell its compute units");
        if ((st = dev_alloc(&s->d_stats_partials, (size_t)slots * STATS_WORDS)) != TR_OK) return st;
        s->stats_slots = slots;
    }
    StatsArgs a = {};
    a.fb = s->d_fb;
    a.fbclean = s->d_fbclean;
    a.z = depth && !cleared ? s->d_z : nullptr;
    a.zclean = depth && !cleared ? s->d_zclean : nullptr;
    a.partials = s->d_stats_partials;
    a.frame = s->frame;
    a.rule = stats_rule(p, s->width, s->height, s->frame.band_y0, s->frame.band_y1);
    a.cleared = cleared ? 1u : 0u;
    // (never more workgroups than slots: the device's count of compute units does not change)
    const uint32_t cap = s->stats_cap ? std::min(s->stats_cap, s->stats_slots) : s->stats_slots;
    return timed_launch(s, K_STATS, "k_stats", [&] { return launch_stats(a, (uint32_t *)out_device, s->stream, cap, &s->stats_grid); });
}

int check_stats_scene(const tr_scene *s)
{
    if (s->broken) return unusable();
    return TR_OK;
}

}  // namespace

int tr_scene_frame_stats(tr_scene *s, const tr_stats_params *p, void *out)
{
    if (!s) return tr::fail(TR_E_INVALID, "tr_scene_frame_stats: null scene");
    int st = check_stats_params(p, s->width, s->height, "tr_scene_frame_stats");
    if (st != TR_OK) return st;
    if (!out) return tr::fail(TR_E_INVALID, "tr_scene_frame_stats: null argument");
    if ((st = check_stats_scene(s)) != TR_OK) return st;
    HIP_TRY(hipSetDevice(s->device));
    void *target = nullptr;
    st = classify_out(out, sizeof(tr_frame_stats), "tr_scene_frame_stats", "tr_scene_get_frame_stats", "record", &target);
    if (st == TR_OK && (uintptr_t)target % 4u != 0u) st = tr::fail(TR_E_INVALID, "tr_scene_frame_stats: `out` is not aligned to 4 bytes");
    if (st == TR_OK) st = enqueue_stats(s, p, (uint8_t *)target);
    if (st == TR_OK) handed_on(s);
    return st;
}

int tr_scene_get_frame_stats(tr_scene *s, const tr_stats_params *p, tr_frame_stats *host)
{
    if (!s) return tr::fail(TR_E_INVALID, "tr_scene_get_frame_stats: null scene");
    int st = check_stats_params(p, s->width, s->height, "tr_scene_get_frame_stats");
    if (st != TR_OK) return st;
    if (!host) return tr::fail(TR_E_INVALID, "tr_scene_get_frame_stats: null argument");
    if ((st = check_stats_scene(s)) != TR_OK) return st;
    return get_stage(s, (uint8_t *)host, sizeof(tr_frame_stats), nullptr, [&](uint8_t *o) { return enqueue_stats(s, p, o); });
}

// The rule of tr_stats.h over a caller's arrays, on the host.  Needs no GPU.
int tr_frame_stats_host(uint32_t width, uint32_t height, const uint8_t *rgb, const float *z, const tr_stats_params *p, tr_frame_stats *out)
{
    int st = check_stats_params(p, width, height, "tr_frame_stats_host");
    if (st != TR_OK) return st;
    if (!out) return tr::fail(TR_E_INVALID, "tr_frame_stats_host: null argument");
    const bool empty = width == 0u || height == 0u;
    if (!empty && (!rgb || ((p->flags & TR_STATS_DEPTH) && !z))) return tr::fail(TR_E_INVALID, "tr_frame_stats_host: null argument");
    stats_host(width, height, rgb, z, stats_rule(p, width, height, 0, (int32_t)height), reinterpret_cast<StatsRecord *>(out));
    return TR_OK;
}

int tr_frame_stats_merge(tr_frame_stats *dst, const tr_frame_stats *src)
{
    if (!dst || !src) return tr::fail(TR_E_INVALID, "tr_frame_stats_merge: null argument");
    if (dst == src) return tr::fail(TR_E_INVALID, "tr_frame_stats_merge: dst is src (the two pixel sets are disjoint)");
    stats_merge(reinterpret_cast<StatsRecord *>(dst), reinterpret_cast<const StatsRecord *>(src));
    return TR_OK;
}

int tr_scene_debug_stats_grid(tr_scene *s, uint32_t cap)
{
    if (!s) return tr::fail(TR_E_INVALID, "tr_scene_debug_stats_grid: null scene");
    s->stats_cap = cap;
    return (int)s->stats_grid;
}

int tr_scene_band_tiles(tr_scene *s, const void *frame_buffer_device, tr_band_tiles *out)
{
    if (!s || !out) return tr::fail(TR_E_INVALID, "null argument");
    HIP_TRY(hipSetDevice(s->device));
    int st = flush_clear_color(s);
    if (st != TR_OK) return st;
    st = submit_pending(s);
    if (st != TR_OK) return st;
    const uint8_t *fb = frame_buffer_device ? (const uint8_t *)frame_buffer_device : s->d_fb;
    const uint32_t *clean = nullptr;
    for (const tr_scene::FbFlags &f : s->fb_flags)
        if (f.fb == fb) clean = f.clean;
    if (!clean) return tr::fail(TR_E_INVALID, "tr_scene_band_tiles: the scene has not rendered into this frame buffer");
    out->frame_buffer_device = fb;
    out->clean_device = clean;
    out->width = s->frame.width;
    out->height = s->frame.height;
    out->tiles_x = s->frame.ntx;
    out->tiles_y = s->frame.nty;
    out->first_tile_row = s->frame.ty_base;
    out->band_y0 = s->frame.band_y0;
    out->band_y1 = s->frame.band_y1;
    handed_on(s);  // (the flags count as read by a consumer)
    s->quiescent = false;
    return TR_OK;
}

void *tr_host_alloc(size_t bytes)
{
    void *p = nullptr, *d = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocMapped) != hipSuccess) return nullptr;
    if (hipHostGetDevicePointer(&d, p, 0) != hipSuccess) d = nullptr;
    if (d) {
        std::lock_guard<std::mutex> lock(g_host_mutex);
        g_host_allocs[p] = { bytes, d, ++g_host_serial, 0u, 0u };
    }
    return p;
}

void tr_host_free(void *p)
{
    if (!p) return;
    {
        std::lock_guard<std::mutex> lock(g_host_mutex);
        g_host_allocs.erase(p);
    }
    (void)hipHostFree(p);
}

int tr_scene_host_buffer_written(tr_scene *s, void *p)
{
    if (!s || !p) return tr::fail(TR_E_INVALID, "null argument");
    // nobody's record of the buffer holds any more (this scene's, and any other scene's that reads back into it)
    std::lock_guard<std::mutex> lock(g_host_mutex);
    auto it = g_host_allocs.find(p);
    if (it != g_host_allocs.end()) {
        it->second.writer = 0u;
        it->second.gen += 1u;
    }
    return TR_OK;
}

int tr_scene_get_z_buffer(tr_scene *s, uint8_t *rgb)
{
    if (!s || !rgb) return tr::fail(TR_E_INVALID, "null argument");
    int fst = sync_and_status(s);
    if (fatal(fst)) return fst;
    int st = s->z_fb_cleared ? TR_OK : ensure_depth(s);
    if (st == TR_OK) st = flush_clear_color(s);
    if (st == TR_OK) st = materialize_depth(s);
    if (st != TR_OK) return st;
    return depth_view(s, fst, s->d_z, rgb);
}

int tr_scene_get_shadow_buffer(tr_scene *s, uint8_t *rgb)
{
    if (!s || !rgb) return tr::fail(TR_E_INVALID, "null argument");
    int fst = sync_and_status(s);
    if (fatal(fst)) return fst;
    int st = flush_clear_shadow(s);
    if (st == TR_OK) st = materialize_shadow(s);
    if (st != TR_OK) return st;
    return depth_view(s, fst, s->d_shadow, rgb);
}

int tr_scene_read_z_f32(tr_scene *s, float *out)
{
    if (!s || !out) return tr::fail(TR_E_INVALID, "null argument");
    int fst = sync_and_status(s);
    if (fatal(fst)) return fst;
    int st = s->z_fb_cleared ? TR_OK : ensure_depth(s);
    if (st == TR_OK) st = flush_clear_color(s);
    if (st == TR_OK) st = materialize_depth(s);
    if (st != TR_OK) return st;
    return finish_read_back(s, fst, out, s->d_z, (size_t)s->width * s->height * 4);
}

int tr_scene_read_shadow_f32(tr_scene *s, float *out)
{
    if (!s || !out) return tr::fail(TR_E_INVALID, "null argument");
    int fst = sync_and_status(s);
    if (fatal(fst)) return fst;
    int st = flush_clear_shadow(s);
    if (st == TR_OK) st = materialize_shadow(s);
    if (st != TR_OK) return st;
    return finish_read_back(s, fst, out, s->d_shadow, (size_t)s->width * s->height * 4);
}

int tr_scene_read_winner_u32(tr_scene *s, uint32_t *out)
{
    if (!s || !out) return tr::fail(TR_E_INVALID, "null argument");
    if (!s->d_winner) return tr::fail(TR_E_INVALID, "scene was created without TR_OPT_WINNER_TAP");
    int fst = sync_and_status(s);
    if (fatal(fst)) return fst;
    int st = flush_clear_color(s);
    if (st != TR_OK) return st;
    return finish_read_back(s, fst, out, s->d_winner, (size_t)s->width * s->height * 4);
}

int tr_scene_debug_tile_stamps(tr_scene *s, uint64_t *out, uint32_t cap_tiles)
{
    if (!s || !out) return tr::fail(TR_E_INVALID, "null argument");
    if (!s->d_stamps) return tr::fail(TR_E_INVALID, "scene was created without TR_OPT_TILE_STAMPS");
    if (cap_tiles < s->n_tiles) return tr::fail(TR_E_INVALID, "buffer too small");
    HIP_TRY(hipSetDevice(s->device));
    {
        int sp = submit_pending(s);
        if (sp != TR_OK) return sp;
    }
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipMemcpy(out, s->d_stamps, (size_t)s->n_tiles * 64, hipMemcpyDeviceToHost));
    return (int)s->n_tiles;
}

int tr_scene_profile_enable(tr_scene *s, int on)
{
    if (!s) return tr::fail(TR_E_INVALID, "null scene");
    HIP_TRY(hipSetDevice(s->device));
    {
        int sp = submit_pending(s);
        if (sp != TR_OK) return sp;
    }
    HIP_TRY(hipStreamSynchronize(s->stream));
    drain_events(s);
    s->profiling = on != 0;
    if (on) {
        memset(s->prof_ms, 0, sizeof s->prof_ms);
        memset(s->prof_n, 0, sizeof s->prof_n);
        memset(s->prof_frames, 0, sizeof s->prof_frames);
        s->frame_intervals_us.clear();
    }
    return TR_OK;
}

int tr_scene_profile_read(tr_scene *s, tr_kernel_time *out, int cap)
{
    if (!s || !out || cap <= 0) return tr::fail(TR_E_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(s->device));
    {
        int sp = submit_pending(s);
        if (sp != TR_OK) return sp;
    }
    HIP_TRY(hipStreamSynchronize(s->stream));
    drain_events(s);
    int n = 0;
    for (int k = 0; k < K_COUNT && n < cap; k++) {
        if (s->prof_n[k] == 0) continue;
        memset(&out[n], 0, sizeof out[n]);
        strncpy(out[n].name, kKernelNames[k], sizeof out[n].name - 1);
        out[n].launches = s->prof_n[k];
        out[n].total_ms = s->prof_ms[k];
        out[n].frames = s->prof_frames[k];
        n++;
    }
    return n;
}

int tr_scene_profile_frame_intervals(tr_scene *s, float *out_us, int cap)
{
    if (!s || !out_us || cap <= 0) return tr::fail(TR_E_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(s->device));
    {
        int sp = submit_pending(s);
        if (sp != TR_OK) return sp;
    }
    HIP_TRY(hipStreamSynchronize(s->stream));
    drain_events(s);
    const int n = (int)s->frame_intervals_us.size() < cap ? (int)s->frame_intervals_us.size() : cap;
    memcpy(out_us, s->frame_intervals_us.data(), (size_t)n * sizeof(float));
    return n;
}

}  // extern "C"
