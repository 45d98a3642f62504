/*
 * tiny_renderer.h -- C ABI of the MI355X-native triangle-fill path.
 *
 * Drop-in boundary: the reference has no FFI; its caller (src/app.rs:137-146,170,208-213)
 * talks to the Rust methods of `Scene` (src/scene.rs:44-269).  Each entry point below names the
 * method it replaces.  A Rust host binds these with an `extern "C"` block;
 * everything is plain pointers, sizes and int status codes -- no exceptions cross this line.
 *
 * Call protocol per frame, as in app.rs:170,208-213:
 *     tr_scene_clear -> tr_scene_set_light_direction -> tr_scene_set_camera ->
 *     tr_scene_render -> tr_scene_get_frame_buffer
 * `render` does not clear; calling it twice without `clear` depth-tests against the previous
 * result exactly like the reference.  A tr_scene is not thread-safe (the reference's Scene is
 * not even Send, shader.rs:85-87).  All rendering runs on the GPU; there is no CPU fallback:
 * tr_scene_create fails with TR_E_HIP when no gfx950 device is usable.
 */
#ifndef TINY_RENDERER_H
#define TINY_RENDERER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: what this header declares is all it exports. */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define TR_ABI_VERSION 3   /* 3: tr_options.max_frame_slots, TR_OPT_STORE_DEPTH, tr_exchange_set_ranges, 64 exchange slots */

/* Status codes.  0 = ok, negative = failure (the reference panics at the cited site). */
enum {
    TR_OK = 0,
    TR_E_INVALID = -1,          /* bad argument / NULL handle */
    TR_E_UNKNOWN_PIPELINE = -2, /* shader.rs:108 */
    TR_E_BAD_POLYGON = -3,      /* scene.rs:218, or an index outside positions/tex_coords/normals */
    TR_E_SINGULAR = -4,         /* try_inverse().unwrap(): shader.rs:224,277,278,631; :921 */
    TR_E_OOB_LOOKUP = -5,       /* device error word: texture / shadow-buffer index out of range
                                   (util.rs:40,52,68,82; shader.rs:778,912,935) or w == 0
                                   (shader.rs:158); the frame is produced but parity is undefined */
    TR_E_HIP = -6,              /* HIP runtime failure or no usable device */
    TR_E_IO = -7,               /* file missing / unreadable (app.rs:94,99: `?`) */
    TR_E_FORMAT = -8,           /* unsupported OBJ / TGA content */
    TR_E_BIN_OVERFLOW = -9,     /* the (polygon, screen tile) pairs of one pass exceeded the record pool AND the frame
                                   could not be rendered again behind the caller's back (see tr_scene_sync); the
                                   pool has been grown: render the frame again, or size it with
                                   tr_options.bin_capacity.  No single tile has a capacity. */
    TR_E_NOMEM = -10,
    TR_E_EXCHANGE = -11,        /* multi-GPU frame exchange: a peer's band did not arrive */
    TR_E_RCCL = -12             /* RCCL backend of the frame exchange: librccl missing or a collective failed */
};

/* obj::raw::RawObj as the path reads it (util.rs:25-31, shader.rs:136-147,363-367,
 * scene.rs:216-226).  Indices are zero based; a polygon contributes its first three
 * (position, tex_coord, normal) triples. */
typedef struct tr_mesh {
    const float *pos;    /* n_pos * 3  (obj-rs keeps a 4th w component; the path ignores it) */
    const float *tex;    /* n_tex * 3 */
    const float *nrm;    /* n_nrm * 3 */
    const uint32_t *idx; /* n_tri * 9 : p0,t0,n0, p1,t1,n1, p2,t2,n2 */
    uint32_t n_pos, n_tex, n_nrm, n_tri;
} tr_mesh;

/* image::RgbImage: tightly packed rgb8, row 0 = top of the picture. */
typedef struct tr_image_rgb8 {
    const uint8_t *rgb;
    uint32_t w, h;
} tr_image_rgb8;

#define TR_OPT_WINNER_TAP 0x1u /* keep a per-pixel winning-polygon index (parity tap) */
#define TR_OPT_TILE_STAMPS 0x2u /* diagnostic: record per-tile start/end clocks of the last pass */
#define TR_OPT_NO_AUTO_GROUP 0x4u /* tr_scene_render submits every frame on its own (see tr_scene_render) */
/* A caller's frame buffers (tr_options.frame_buffer_device, tr_scene_set_frame_buffer_device, tr_scene_render_frames)
 * are written by nobody but the scene while they are its targets -- apart from rows outside the scene's band.  The
 * scene then keeps, per buffer, which tiles already hold the cleared colour, and a cleared frame does not store the
 * zeros of an empty tile again (a caller that double-buffers frames for an exchange: most of the frame, every frame).
 * Without the flag nothing is remembered about a caller's buffer from one tr_scene_set_frame_buffer_device /
 * tr_scene_render_frames call to the next: whatever wrote it in between -- a post-process, a memset, an allocator
 * handing the address to another tensor -- a cleared render produces every pixel of its band. */
#define TR_OPT_TRUST_FRAME_BUFFERS 0x8u
/* Transient depth off.  By default the colour pass of a CLEARED frame resolves its depth on the chip and does not write
 * it to the z buffer: nothing reads the z buffer of such a frame -- the next cleared frame overwrites it unseen -- and the
 * first consumer that does want it (tr_scene_get_z_buffer / tr_scene_read_z_f32, or a tr_scene_render without a clear,
 * which depth-tests against it: scene.rs:151) gets it from a repeat of the pass for the depth alone, so that what
 * callers observe is unchanged.  With this flag every colour pass writes its depth, as the reference's does. */
#define TR_OPT_STORE_DEPTH 0x10u

typedef struct tr_options {
    uint32_t struct_size;      /* = sizeof(tr_options) */
    int32_t device;            /* HIP device ordinal; -1 = current device */
    uint32_t flags;            /* TR_OPT_* */
    /* Screen-band shard (multi-GPU): this scene renders only output-image rows
     * [band_row0, band_row1) (row 0 = top, as returned by get_frame_buffer).
     * 0,0 = the whole frame. */
    uint32_t band_row0, band_row1;
    void *stream;              /* hipStream_t to enqueue on; NULL = library-owned stream */
    void *frame_buffer_device; /* device pointer to 3*W*H bytes to render into (e.g. the
                                  all-gather buffer); NULL = library-owned */
    uint64_t bin_capacity;     /* records in a pass's pool = (polygon, 128x16 screen tile) pairs of one pass of one
                                  frame; every tile gets exactly the records it needs from it.  0 = automatic:
                                  twice an estimate from the frame size and the polygon count -- polygons with
                                  boxes of side s = sqrt(2 W H / n) meet (1 + s/128)(1 + s/16) tiles each, half
                                  of them face the viewer -- at least 65 536 and at most 16 Mi records.  A pass
                                  that needs more grows the pools and the frame is rendered again. */
    uint32_t tile_waves;       /* wavefronts per 128x16 screen tile: 4, 8, 16, or 0 = automatic (more
                                  while the tiles cannot fill the GPU, 4 from 4096x4096 up).
                                  Speed only: results do not depend on it. */
    uint32_t tile_mode;        /* how a tile's wavefronts divide its work: 1 = each owns a column of the tile and
                                  sees every polygon of the bin, 2 = each owns a share of the bin and sees the
                                  whole tile (depth resolve through LDS atomics), 0 = automatic.  The shared mode
                                  (2, pinned or chosen) is honoured up to 2^20 polygons per pass, counted as mesh
                                  polygons x instances; beyond that the pass runs the column kernels (1).
                                  Speed only: results do not depend on it. */
    uint32_t frames_per_launch; /* tr_scene_render_frames: frames rendered by one launch of each kernel (1..32), 0 =
                                  automatic (by tile count: 4 at 4096x4096, 32 for small frames; a call of several
                                  groups uses up to three times that per launch, a call of sixteen groups or more
                                  grows to 32).  Speed only. */
    uint32_t max_frame_slots;  /* upper bound on the scene's frame slots -- complete sets of render targets (z,
                                  colour, shadow buffer: 7 to 11 bytes per pixel each), one per frame of a group in
                                  flight, hence also on the frames per launch: 1..32, 0 = automatic (as many as the
                                  largest group, up to 32 within 8 GiB; a device without room for that falls back to
                                  the usual group by itself).  For callers that keep many scenes on one GPU. */
} tr_options;

typedef struct tr_scene tr_scene;

/* Scene::new (scene.rs:47-88).  tex[] = texture, normal_map, normal_map_tangent, specular_map
 * (the order of Scene::new's arguments).  Inputs are copied (the reference moves them).
 * Pipeline names: shader.rs:100-109 (`true_normal`, README.md:18, is accepted as an alias of
 * `normal_map`). */
int tr_scene_create(uint32_t width, uint32_t height, const tr_mesh *mesh,
                    const tr_image_rgb8 tex[4], const char *pipeline_name,
                    const tr_options *opts, tr_scene **out);
void tr_scene_destroy(tr_scene *s);

int tr_scene_clear(tr_scene *s);                                  /* scene.rs:128-137 */
int tr_scene_set_light_direction(tr_scene *s, const float v[3]); /* scene.rs:140-142 */
int tr_scene_set_camera(tr_scene *s, const float look_from[3], const float look_at[3],
                        const float up[3]);                       /* scene.rs:145-149 */
/* scene.rs:151-268.  Asynchronous.  On the library's own stream a render that follows a clear may be held back
 * on the host until a few such frames have been issued (tr_scene_frames_per_launch) and is then rendered
 * together with them by fused kernel launches (as tr_scene_render_frames does; only the last frame's targets
 * are the scene's, which is all the per-frame protocol lets anybody see).  Every getter, tr_scene_sync,
 * tr_scene_flush and tr_scene_get_frame_buffer_async submit what is held back first, so a frame that is read
 * right after its render goes to the device alone, at once. */
int tr_scene_render(tr_scene *s);
int tr_scene_set_auto_group(tr_scene *s, int on); /* the same switch as TR_OPT_NO_AUTO_GROUP, at run time */

/* Many frames per call -- the throughput path (nothing of the kind upstream, whose caller renders one frame per
 * window refresh, app.rs:170-213).  Frame i of the call is exactly what
 *     tr_scene_clear; tr_scene_set_light_direction(frames[i].light);
 *     tr_scene_set_camera(frames[i].look_from, .look_at, .up); tr_scene_render
 * produces, but the frames of a group (tr_scene_frames_per_launch of them) are rendered TOGETHER, by one launch of
 * each kernel: a lone frame leaves the GPU draining for a third of its tile kernel at 4096x4096, and a small frame
 * never fills it.  Each frame of a group has render targets of its own ("frame slots": z, colour, shadow buffer),
 * handed out in rotation, so when the call returns its LAST tr_scene_frames_per_launch frames exist
 * (tr_scene_frames_kept).  The scene is left as the per-frame calls would leave it: light and camera of the last
 * frame, the last frame current for every getter and for a later tr_scene_render without clear.
 * frame_buffers_device: NULL (colour into the slots' own buffers) or n_frames device pointers of 3*W*H bytes each,
 * frame i's colour target (e.g. the all-gather buffers of a multi-GPU caller); a buffer belongs to the scene as in
 * tr_scene_set_frame_buffer_device.  Asynchronous like tr_scene_render: on a caller's stream all the frames'
 * kernels are enqueued when the call returns. */
typedef struct tr_frame_params {
    float light[3];
    float look_from[3], look_at[3], up[3];
} tr_frame_params;
int tr_scene_render_frames(tr_scene *s, uint32_t n_frames, const tr_frame_params *frames, void *const *frame_buffers_device);
/* Instanced rendering (nothing of the kind upstream): draw the scene's mesh many times, each copy placed by one entry
 * of a table.  Instance k draws every polygon of the mesh with each position component p replaced by
 *     fl(fl(p * scale) + offset)         -- a multiply, then an add, each rounded once (no fused multiply-add)
 * and the mesh's own normals and texture coordinates.  Polygons are drawn in instance-major order: instance k,
 * triangle t is polygon k * n_tri + t -- the winner tap, the depth test's tie order and the culling see the mesh
 * concatenated n_instances times.  So a scene with table T renders bit for bit what a scene created from that
 * concatenated, host-transformed mesh renders, in every pipeline.  No rotations: normals are not transformed (for
 * those, tr_instance_xform below).
 * n_instances == 0 (instances may then be NULL) draws the mesh itself, untransformed -- the default, and NOT the same as
 * one instance {0, 0, 0, 1}: -0.0 * 1 + 0 is +0.0.  n_tri * n_instances must stay below 0xFFFFFFF0 (TR_E_INVALID).
 * The table is scene state like the camera: renders issued after the call draw it; frames issued before (also those
 * tr_scene_render holds back to fuse) keep the one they were issued with.  It is copied: the caller may reuse its
 * memory at once.  A table larger than the scene has seen grows the scene's record pools as tr_scene_create would
 * size them for the concatenated mesh (and waits for the scene's queued work to do so).  Errors change nothing. */
typedef struct tr_instance {
    float offset[3];
    float scale;
} tr_instance; /* 16 bytes */
int tr_scene_set_instances(tr_scene *s, uint32_t n_instances, const tr_instance *instances);
/* tr_scene_render_frames with a table per frame: frame i is exactly
 *     tr_scene_set_instances(s, n_instances, instances + i * n_instances); tr_scene_clear; set_light_direction;
 *     set_camera; tr_scene_render
 * (still one fused launch per kernel for the frames of a group).  The scene is left with the last frame's table
 * current; tr_scene_select_frame makes a kept frame's table current with its light and camera.  Plain
 * tr_scene_render_frames draws the scene's current table in every frame. */
int tr_scene_render_frames_instanced(tr_scene *s, uint32_t n_frames, const tr_frame_params *frames, uint32_t n_instances,
                                     const tr_instance *instances /* n_frames * n_instances */,
                                     void *const *frame_buffers_device);
/* Instance transforms: the second kind of instance table, for copies that are turned, sheared, scaled per axis or
 * mirrored.  Instance k draws every polygon of the mesh with each position (x, y, z) and each vertex normal (a, b, c)
 * replaced, component r = 0..2, by
 *     p'_r = fl( fl( fl( fl(m[4r]*x) + fl(m[4r+1]*y) ) + fl(m[4r+2]*z) ) + m[4r+3] )
 *     n'_r = fl( fl( fl(n[3r]*a) + fl(n[3r+1]*b) ) + fl(n[3r+2]*c) )
 * -- every multiply and every add rounded once, in this order; no fused multiply-add.  Texture coordinates are the
 * mesh's own, the polygon order is instance-major as for tr_instance.  So a scene with table T renders, bit for bit and
 * in every pipeline, what a scene created from the concatenated mesh transformed this way on the host renders
 * (tr_instance_transform_mesh builds its positions and normals); a mirroring entry (det < 0) flips the winding and with
 * it the culling, exactly as it does for that mesh.
 * `n` is the caller's: the library does not derive it from `m`.  The reference normalises every transformed normal
 * (shader.rs:368-371, 562-584), so any positive multiple of the inverse transpose of m's linear part gives the same
 * picture up to rounding.
 * Object-space normal maps do not turn: the closures of `normal_map` and `specular` take their normal from
 * normal_map.tga in object space (util.rs:51-56), so those two pipelines light a turned instance as if it were not
 * turned (their geometry, depth and culling do follow m).  `default`, `phong`, `darboux`, `shadow` and `occlusion`
 * follow the transform through positions and vertex normals.
 * One table at a time: a scene has one table, of either kind; setting one kind replaces the other, and n_instances == 0
 * in either call draws the mesh itself.  Everything else -- the copy, frames issued earlier keeping their table, pool
 * growth, the limit n_tri * n_instances < 0xFFFFFFF0, errors changing nothing -- is as for tr_scene_set_instances. */
typedef struct tr_instance_xform {
    float m[12];   /* position transform, row-major 3 x 4: row r = m[4r+0..2] (linear part), m[4r+3] (translation) */
    float n[9];    /* normal transform, row-major 3 x 3 */
    float pad[3];  /* ignored; keeps entries 16-byte aligned (six 16-byte loads) */
} tr_instance_xform; /* 96 bytes */
int tr_scene_set_instance_transforms(tr_scene *s, uint32_t n_instances, const tr_instance_xform *table);
/* tr_scene_render_frames_instanced for transform tables: frame i draws table + i * n_instances; one fused launch per
 * kernel for the frames of a group; the last frame's table is left current, tr_scene_select_frame restores a kept
 * frame's. */
int tr_scene_render_frames_transformed(tr_scene *s, uint32_t n_frames, const tr_frame_params *frames, uint32_t n_instances,
                                       const tr_instance_xform *table /* n_frames * n_instances */,
                                       void *const *frame_buffers_device);
/* The rule above on the host (no GPU needed, like tr_prepare_uniforms): positions and normals of the concatenated mesh
 * that `table` draws, instance-major, computed by the very inline function the vertex stage calls.  mesh->tex and
 * mesh->idx are not read. */
int tr_instance_transform_mesh(const tr_mesh *mesh, uint32_t n_instances, const tr_instance_xform *table,
                               float *pos_out /* n_instances*n_pos*3 */, float *nrm_out /* n_instances*n_nrm*3 */);
/* Morph targets (blend shapes; nothing of the kind upstream, whose mesh is frozen at Scene::new): the SHAPE of the mesh
 * per frame.  A scene gets T targets, 1 <= T <= TR_MORPH_MAX_TARGETS (an interface limit, not a measured one); each is
 * a set of deltas laid out like the mesh's own arrays -- dpos: n_pos * 3 floats, dnrm: n_nrm * 3 floats.  A pose is a
 * weight vector w[0..T).  Every position component p with deltas d_k, and in the same way every normal component, is
 * drawn as
 *     v = p
 *     for k = 0 .. T-1, in this order, skipping every k with w[k] == 0.0f (either sign):
 *         v = fl( v + fl( w[k] * d_k ) )          -- one multiply, one add, each rounded once; no fused multiply-add
 * Texture coordinates and indices are the mesh's own.  Skipping zero weights is part of the rule: a pose of zeros is
 * the mesh itself bit for bit, -0.0 components and targets holding inf or nan included.  Normals are not renormalised
 * (the reference normalises every transformed normal, shader.rs:368-371, 562-584).  So a scene under pose w renders,
 * bit for bit and in every pipeline, what a scene created from the host-morphed mesh (tr_morph_mesh) renders.
 * Object-space normal maps do not deform -- the caveat of tr_instance_xform: `normal_map` and `specular` follow the
 * deformation in geometry, depth and culling but take their light from normal_map.tga.
 * tr_scene_set_morph_targets copies the deltas (dpos: n_targets * n_pos * 3 floats, dnrm: n_targets * n_nrm * 3,
 * target-major), gathers them per polygon as the mesh was and uploads them once; n_targets == 0 (the arrays may then be
 * NULL) drops the targets and the current pose.  It waits for the scene's queued work.  New targets leave the scene
 * without a pose as well (a pose belongs to the targets it was set under); frames already rendered are what they are.
 * tr_scene_set_morph_weights: the pose is scene state like the camera -- renders issued after the call draw it, frames
 * issued before (also those tr_scene_render holds back to fuse) keep theirs.  n_weights must be 0 or T; 0 draws the
 * mesh itself straight from its own rows (no blend kernel runs).  The weights are copied.
 * Morphing composes with instancing: the pose deforms the mesh, then the scene's current table, of either kind, places
 * or turns the deformed mesh -- polygon order, winner tap, tie order and culling are those of the concatenated,
 * host-morphed-then-transformed mesh.  One pose per frame applies to all instances.
 * Errors (T above the limit, a weight count that is neither 0 nor T, a NULL where data is required) are TR_E_INVALID
 * and change nothing. */
#define TR_MORPH_MAX_TARGETS 64
int tr_scene_set_morph_targets(tr_scene *s, uint32_t n_targets, const float *dpos, const float *dnrm);
int tr_scene_set_morph_weights(tr_scene *s, uint32_t n_weights, const float *w);
/* tr_scene_render_frames with a pose per frame: frame i is exactly
 *     tr_scene_set_morph_weights(s, n_weights, weights + i * n_weights); tr_scene_clear; set_light_direction;
 *     set_camera; tr_scene_render
 * (still one fused launch per kernel for the frames of a group; their poses are blended by one launch of k_morph ahead
 * of it).  The last frame's pose is left current; tr_scene_select_frame makes a kept frame's pose current with its light
 * and camera.  The scene's current instance table applies to every frame.  Plain tr_scene_render_frames, _instanced and
 * _transformed draw the current pose in every frame. */
int tr_scene_render_frames_morphed(tr_scene *s, uint32_t n_frames, const tr_frame_params *frames, uint32_t n_weights,
                                   const float *weights /* n_frames * n_weights */, void *const *frame_buffers_device);
/* Diagnostic: sets of posed rows (n_tri * 96 bytes each) the scene has on the device now -- those of the poses its frame
 * slots, kept frames, held-back frames and current state hold, and free ones waiting to be used again.  Bounded by the
 * frame slots plus the frames in flight, whatever the length of a tr_scene_render_frames_morphed call; free ones go back
 * to the device beyond a group's worth and at tr_scene_set_morph_targets. */
int tr_scene_debug_morph_rows(tr_scene *s);
/* The rule above on the host (no GPU needed): positions and normals of `mesh` under pose w (n_targets weights),
 * computed by the very inline function k_morph calls.  mesh->tex and mesh->idx are not read. */
int tr_morph_mesh(const tr_mesh *mesh, uint32_t n_targets, const float *dpos, const float *dnrm, const float *w,
                  float *pos_out /* n_pos*3 */, float *nrm_out /* n_nrm*3 */);
/* Skinning (articulated deformation; nothing of the kind upstream): bones move the mesh per frame.  A skin gives every
 * POSITION INDEX P of the mesh TR_SKIN_INFLUENCES = 4 pairs (bone index, weight); a palette is n_bones entries of
 * tr_instance_xform -- m for positions, n for normals, pad ignored -- with 1 <= n_bones <= TR_SKIN_MAX_BONES (an
 * interface limit, not a measured one).  Corner i of a polygon, with position p at position index P and normal a at its own
 * normal index, is drawn as
 *     acc = none
 *     for j = 0 .. 3, in this order, skipping every j with weight[P][j] == 0.0f (either sign):
 *         q   = palette[bone[P][j]].m applied to p      -- the rule of tr_instance_xform above, unchanged
 *         t_r = fl( weight[P][j] * q_r )                -- r = 0..2
 *         acc_r = (acc is none) ? t_r : fl( acc_r + t_r )
 *     p' = (acc is none) ? p : acc
 * and the normal by the same steps with palette[..].n applied to a -- under the influences of P: OBJ indexes normals
 * separately, so a normal has none of its own.  No fused multiply-add; weights are used as given (the library does not
 * normalise them); normals are not renormalised (the reference normalises every transformed normal).  Hence a corner
 * whose four weights are zero keeps the mesh's own bit patterns, -0.0 included, whatever the palette holds (inf, nan),
 * and a corner with one influence of weight 1.0f gets exactly what an instance-transform table of that one entry draws.
 * Texture coordinates and the polygon order are the mesh's own.  Object-space normal maps do not deform -- the caveat
 * of tr_instance_xform and of morph targets: `normal_map` and `specular` follow the deformation in geometry, depth and
 * culling but take their light from normal_map.tga.
 * Order of composition: the morph pose, if any, deforms the mesh; the palette skins the morphed rows; the scene's
 * current instance table, of either kind, then places the result.
 * tr_scene_set_skin copies bone and weight (n_pos * 4 each), gathers them per polygon as the mesh was and uploads them
 * once; it waits for the scene's queued work and leaves the scene without a palette (the morph pose stays);
 * n_bones == 0 (the arrays may then be NULL) drops the skin.  tr_scene_set_morph_targets leaves the palette current:
 * the skin does not depend on the targets.
 * tr_scene_set_bone_palette: scene state like the morph weights -- copied; renders issued after the call draw it,
 * frames issued before (also held-back ones) keep theirs.  n_bones must be 0 or the skin's count; 0 means no palette:
 * no skin kernel runs and the rows are the morph pose's or the mesh's own.
 * Errors (a bone index >= n_bones, n_bones above the limit or not the skin's, a NULL where data is required) are
 * TR_E_INVALID and change nothing. */
#define TR_SKIN_INFLUENCES 4
#define TR_SKIN_MAX_BONES 128
int tr_scene_set_skin(tr_scene *s, uint32_t n_bones, const uint32_t *bone /* n_pos*4 */, const float *weight /* n_pos*4 */);
int tr_scene_set_bone_palette(tr_scene *s, uint32_t n_bones, const tr_instance_xform *palette);
/* tr_scene_render_frames with a palette per frame: frame i is exactly
 *     tr_scene_set_bone_palette(s, n_bones, palettes + i * n_bones); tr_scene_clear; set_light_direction; set_camera;
 *     tr_scene_render
 * (one fused launch per kernel for the frames of a group; their rows are skinned by one launch of k_skin ahead of it,
 * behind k_morph where there is a morph pose).  The last frame's palette is left current; tr_scene_select_frame
 * restores a kept frame's.  The current morph pose and the current instance table apply to every frame.  Plain
 * tr_scene_render_frames, _instanced, _transformed and _morphed draw the current palette in every frame. */
int tr_scene_render_frames_skinned(tr_scene *s, uint32_t n_frames, const tr_frame_params *frames, uint32_t n_bones,
                                   const tr_instance_xform *palettes /* n_frames * n_bones */, void *const *frame_buffers_device);
/* The rule above on the host (no GPU needed), by the very inline function k_skin calls.  A normal shared by corners
 * with different positions gets different results, so the skinned mesh cannot reuse the mesh's index arrays: the
 * output is unrolled -- corner 3t+i of polygon t gets a position and a normal of its own, idx_out holds per corner
 * {3t+i, the mesh's texture index, 3t+i}; the polygon order is kept and mesh->tex is used as it is.  A scene under a
 * palette renders, bit for bit and in every pipeline, what a scene created from this mesh renders. */
int tr_skin_mesh(const tr_mesh *mesh, uint32_t n_bones, const uint32_t *bone, const float *weight,
                 const tr_instance_xform *palette, float *pos_out /* n_tri*9 */, float *nrm_out /* n_tri*9 */,
                 uint32_t *idx_out /* n_tri*9 */);
int tr_scene_frames_per_launch(tr_scene *s); /* frames per group of this scene */
int tr_scene_frames_kept(tr_scene *s);       /* frames of the last tr_scene_render_frames call that still exist
                                                (0 after a tr_scene_render) */
/* 1 when the scene's newest fused tile launches (the passes of its last group of frames, or a lone cleared frame's
 * colour pass) ran the tile kernels compiled for frames made of whole tiles only -- width a multiple of 128, the band
 * whole tile rows inside the frame -- else 0 (also before the first such launch).  Speed only: the frames are the
 * same either way.  TR_INTERIOR=0 in the environment (read once per process) keeps every launch on the general kernels. */
int tr_scene_interior_tiles(tr_scene *s);
/* Makes the frame `back` frames before the last one of that call (0 = the last) the scene's current frame: getters,
 * tr_scene_frame_buffer_device and later renders refer to its targets, light and camera. */
int tr_scene_select_frame(tr_scene *s, uint32_t back);

/* scene.rs:92-125.  Caller-owned host buffers of 3*W*H bytes, row 0 = top.  Synchronizes.
 * Returns the sticky device status (TR_E_OOB_LOOKUP, TR_E_BIN_OVERFLOW) of the frame. */
int tr_scene_get_frame_buffer(tr_scene *s, uint8_t *rgb);
int tr_scene_get_z_buffer(tr_scene *s, uint8_t *rgb);
int tr_scene_get_shadow_buffer(tr_scene *s, uint8_t *rgb);

/* Parity taps, not in the reference: raw buffers in the reference's internal layout
 * (index = x + y*W, row 0 = bottom), W*H elements. */
int tr_scene_read_z_f32(tr_scene *s, float *out);
int tr_scene_read_shadow_f32(tr_scene *s, float *out);
int tr_scene_read_winner_u32(tr_scene *s, uint32_t *out); /* needs TR_OPT_WINNER_TAP;
                                                             0xFFFFFFFF = no fragment */

/* Streaming frames out (the reference hands every frame to its window, app.rs:213-218): enqueue
 * the device-to-host copy of the frame behind the renders issued so far and return at once; `rgb`
 * (3*W*H bytes, row 0 = top) holds the frame after tr_scene_sync(); a later render is ordered after the copy.
 * Into memory from tr_host_alloc (page-locked, mapped into the device) only what has to travel does: the scene
 * knows which 128x16 tiles of the frame hold the cleared colour, and remembers per host buffer which tiles it
 * has written as zeros there -- those are skipped (widths that are multiples of 16; three quarters of a
 * 4096x4096 frame of the reference's model: 1.1 ms -> 0.3 ms per frame).  The buffer always ends up holding the
 * complete frame: the record of a buffer's zero tiles belongs to the scene that wrote it last and lapses when
 * anybody else writes the buffer -- another scene reading back into it (the library knows), or the caller, who
 * says so with tr_scene_host_buffer_written (no scene then assumes anything about its content); reading it needs
 * nothing.  A band scene (tr_options.band_row0/1) and any other host memory receive the whole frame buffer through
 * the copy engine. */
int tr_scene_get_frame_buffer_async(tr_scene *s, uint8_t *rgb);
void *tr_host_alloc(size_t bytes); /* page-locked host memory mapped into the device, NULL on failure */
void tr_host_free(void *p);
int tr_scene_host_buffer_written(tr_scene *s, void *p);

/* Supersampled output (nothing of the kind upstream, which takes one sample per pixel): the scene's current frame,
 * rendered at W x H, box-filtered on the device by factor f = 2, 4 or 8 into a frame of W/f x H/f pixels, tightly
 * packed rgb8, row 0 = top.  With F the image tr_scene_get_frame_buffer would return,
 *     out[Y][X][c] = ( sum over dy, dx in [0, f) of F[f*Y + dy][f*X + dx][c]  +  f*f/2 ) / (f*f)     (integer division)
 * -- the stored u8 values, per channel, rounded half up; no gamma, no weights.  "Current frame" is what the getters
 * mean: the last render's, a frame chosen with tr_scene_select_frame, the caller's buffer after
 * tr_scene_set_frame_buffer_device.  W and H must be multiples of f, and so must tr_options.band_row0/1 of a band
 * scene (a block of f x f pixels then never straddles a 128x16 tile or the band); anything else is TR_E_INVALID and
 * changes nothing.  Tiles the scene knows to hold the cleared colour are not read (k_resolve stores their zeros).
 * tr_scene_resolve is asynchronous like tr_scene_get_frame_buffer_async: it submits what tr_scene_render holds back and
 * enqueues the resolve behind the renders issued so far; a later render is ordered after it; `out` holds the result
 * after tr_scene_sync.  `out`: 3*(W/f)*(H/f) bytes of device memory, or memory from tr_host_alloc (the kernel then
 * stores through the mapped address: only the resolved frame crosses to the host); other host memory is TR_E_INVALID.
 * A whole-frame scene writes every byte of `out` on every call; a band scene writes output rows
 * [band_row0/f, band_row1/f) and nothing else, so the ranks of a sharded frame can resolve into one buffer.
 * tr_scene_get_resolved takes any host memory, synchronizes and returns the frame's sticky status like
 * tr_scene_get_frame_buffer (rows outside a band scene's band are zeros). */
int tr_scene_resolve(tr_scene *s, uint32_t factor, void *out);
int tr_scene_get_resolved(tr_scene *s, uint32_t factor, uint8_t *rgb);

/* Depth compositing (nothing of the kind upstream, whose Scene draws one mesh with one set of textures through one
 * pipeline): the current frame of scene `src` is merged into the current frame of scene `dst` on the device, by the
 * reference's own depth test (`if z_value <= z_buffer[index] { return false }`, shader.rs:175).  Per pixel, with zs and
 * zd the z values tr_scene_read_z_f32 would return for src and dst:
 *     covered = bits(zs) != bits(f32::MIN)    -- a pixel still at the cleared value was not drawn, and a drawn pixel never
 *                                                holds that value: a fragment at f32::MIN fails the test against it
 *     wins    = covered && !(zs <= zd)
 * Where `wins`, dst's colour becomes src's three bytes, dst's z becomes zs and, if dst has the winner tap, its winner word
 * becomes src's + winner_base (u32, wrapping); elsewhere dst is untouched.  Ties keep dst: the order of the calls is the
 * tie order, as the polygon order is inside one scene.  NaN depth follows the test as written: a comparison with a NaN is
 * false, so a covered src pixel whose z is NaN wins, and so does any covered src pixel over a NaN in dst.
 * What it equals: the reference's fragment stages discard nowhere but at that test, so for the pipelines whose closures
 * read nothing but the polygon, the uniforms and the textures -- `default`, `phong`, `normal_map`, `specular`, `darboux` --
 * merging scene(B) into scene(A), same size, camera, light and textures, winner_base = A's polygon count, is bit for bit
 * what one scene of the concatenated mesh A ++ B renders: colour, z and winner index.  `shadow` and `occlusion` merge by
 * the same rule, but their closures read the scene's OWN shadow buffer: after a plain tr_scene_render of each, B casts no
 * shadow on A and the result is not that of a concatenated scene.  For those two, render the passes separately and merge
 * the shadow buffers in between (tr_scene_render_shadow_pass, tr_scene_shadow_merge, tr_scene_render_colour_pass, below):
 * the claim then holds for them as well.  The scenes may differ in mesh, textures, pipeline, instance table, pose and options.
 * Current frame: on both sides what the getters mean -- the last render's, a frame chosen with tr_scene_select_frame, the
 * caller's buffer after tr_scene_set_frame_buffer_device.
 * Pending work: frames tr_scene_render holds back are submitted, on both scenes; a pending clear of dst is made real; the
 * depth of either frame, if it was left on the chip (see TR_OPT_STORE_DEPTH), is fetched by the depth-only repeat of its
 * pass.  Callers who composite every frame should create BOTH scenes with TR_OPT_STORE_DEPTH: the repeat then never runs.
 * A src that is logically cleared (tr_scene_clear and nothing rendered since) covers nothing: the call returns TR_OK and
 * does nothing.
 * Asynchronous: k_composite is enqueued on dst's stream behind src's frame (an event recorded on src's stream), and src's
 * stream then waits for it, so a later render of src cannot overwrite what the merge reads; the result is there after
 * tr_scene_sync(dst).  Both scenes' passes issued so far count as handed on, as after tr_scene_get_frame_buffer_async:
 * neither frame is rendered again behind the caller's back (a bin overflow among them is reported, TR_E_BIN_OVERFLOW).
 * Tiles (128 x 16) in which src drew nothing are skipped on src's fast-clear flags without reading a pixel.
 * Afterwards dst holds a drawn frame with its depth in memory: a tr_scene_render on dst without a clear depth-tests
 * against the merged z as usual, further tr_scene_composite calls layer more scenes in, every getter sees the merged
 * frame.  The shadow buffers are left alone and src is never written.  src's sticky device status stays src's own:
 * tr_scene_sync(src) returns it.
 * TR_E_INVALID, nothing changed and nothing queued: a NULL scene, dst == src, different devices, different width or
 * height, different tr_options.band_row0/1, dst with TR_OPT_WINNER_TAP and src without. */
int tr_scene_composite(tr_scene *dst, tr_scene *src, uint32_t winner_base);
/* The rule above on the host (no GPU needed), by the very inline function k_composite calls: n_pixels pixels, all arrays
 * in one pixel order of the caller's choosing; z_dst, rgb_dst (3 bytes per pixel) and win_dst are updated in place.
 * win_dst may be NULL (no winner words; win_src is then not read). */
int tr_composite_host(size_t n_pixels, float *z_dst, uint8_t *rgb_dst, uint32_t *win_dst /* or NULL */,
                      const float *z_src, const uint8_t *rgb_src, const uint32_t *win_src /* or NULL */,
                      uint32_t winner_base);

/* Shared shadows (nothing of the kind upstream): the two passes of `shadow` and `occlusion` as calls of their own, and the
 * merge of two scenes' shadow buffers between them, so that composited models shade each other.
 * Why it is exact: the reference's light-space pass is a running maximum without culling,
 *     if z_value >= shadow_buffer[index] { shadow_buffer[index] = z_value }          (shader.rs:703, 841)
 * and its shadow matrix depends on the light, look_at, up and the frame size alone (shader.rs:234-255).  So the shadow
 * buffer of the concatenated mesh A ++ B is A's merged with B's by that same test, per pixel of the whole frame, with zs
 * and zd the values tr_scene_read_shadow_f32 would return for src and dst:
 *     if (zs >= zd) zd = zs
 * bit for bit, the sign of a zero included (>= passes between +0.0 and -0.0: src's zero replaces dst's, as B's last
 * zero fragment decides in the concatenated pass); a NaN on either side compares false and dst keeps its value; f32::MIN
 * -- a pixel src never drew -- replaces nothing but f32::MIN.  The colour passes of the two pipelines read nothing shared
 * but that buffer.  Hence, for two scenes A and B on `shadow` or `occlusion` with the same size, light and camera:
 *     tr_scene_clear(A); tr_scene_clear(B);
 *     tr_scene_render_shadow_pass(A); tr_scene_render_shadow_pass(B);
 *     tr_scene_shadow_merge(A, B); tr_scene_shadow_merge(B, A);          -- both now hold the merged buffer
 *     tr_scene_render_colour_pass(A); tr_scene_render_colour_pass(B);
 *     tr_scene_composite(A, B, n_tri(A));
 * leaves in A, bit for bit, what one scene of A ++ B renders: colour, z, winner index and shadow buffer.
 *
 * tr_scene_render_shadow_pass runs pass 0 of the scene's pipeline -- the light-space depth pass -- into the current
 * frame's shadow buffer, under the current light, look_at, up and instance table / pose / palette.  It consumes a pending
 * shadow clear (tr_scene_clear); a pending clear of z and colour stays pending.  Without a pending clear it raises the
 * buffer as it stands, as tr_scene_render without a clear does.
 * tr_scene_render_colour_pass runs the last pass against the shadow buffer as it stands -- looked up under the shadow
 * matrix the buffer was last rendered, or merged, under.  It consumes the pending clear of z and colour; without one it
 * depth-tests against the frame so far, whose depth is made real first as tr_scene_render does (TR_OPT_STORE_DEPTH).
 *     tr_scene_clear; tr_scene_render_shadow_pass; tr_scene_render_colour_pass
 * is in every byte -- colour, z, winner words, shadow buffer -- what tr_scene_clear; tr_scene_render produces.
 * Both calls are asynchronous, submit first whatever tr_scene_render holds back, and are never held back or fused
 * themselves.  Their passes count as handed on, as after tr_scene_composite: a bin overflow in one is reported by
 * tr_scene_sync (TR_E_BIN_OVERFLOW, the pools grown: issue the calls again), never repaired by rendering the scene's
 * last tr_scene_render again, which would run the scene's own shadow pass over a merged buffer.  tr_scene_render itself
 * is unchanged.  A scene on a one-pass pipeline: TR_E_INVALID, nothing changed.
 *
 * tr_scene_shadow_merge merges src's current shadow buffer into dst's by the rule above.  The shadow buffer is the whole
 * frame on a band scene as well (lookups are in light space, shader.rs:774-778), so the scenes' bands need not match.
 * A src whose shadow buffer is logically cleared (tr_scene_clear and no shadow pass since): TR_OK, nothing happens.  A
 * pending shadow clear of dst is made real first: dst then takes src's buffer.  Asynchronous: k_shadow_merge is enqueued
 * on dst's stream behind src's work (an event recorded on src's stream), and src's stream then waits for it, so a later
 * render of src cannot overwrite what the merge reads; the result is there after tr_scene_sync(dst).  Both scenes' passes
 * issued so far count as handed on.  src is never written; colour, z and winner words of both scenes are untouched.
 * Tiles (128 x 16) whose src fast-clear flag is up are skipped without reading a pixel; a dst tile behind its flag takes
 * src's values without its stale memory being read.
 * Each scene remembers the 16 floats of the shadow matrix its shadow buffer was last rendered under (tr_scene_render and
 * the frame-group calls set them too; a merge into a cleared buffer hands src's on).
 * TR_E_INVALID with a tr_last_error text, nothing changed and nothing queued: a NULL scene, dst == src, different devices,
 * different width or height, either scene on a one-pass pipeline, shadow matrices that differ in any bit -- buffers taken
 * under different lights do not merge into anything meaningful.  The matrices are compared only when BOTH current shadow
 * buffers have one: a buffer no shadow pass has filled (a new scene's zeros, a frame slot not rendered into yet) or a dst
 * with a pending clear merges under any light and takes over src's matrix.
 * Out of scope: shadow passes of their own for the frames of a tr_scene_render_frames* group (a group renders both passes
 * of every frame; select a kept frame and merge into that); a one-pass-pipeline scene as a shadow caster -- give its mesh
 * a second scene on `shadow` and use that scene's shadow pass; an oracle of split passes (the oracle renders whole
 * frames: the split is checked against them). */
int tr_scene_render_shadow_pass(tr_scene *s);
int tr_scene_render_colour_pass(tr_scene *s);
int tr_scene_shadow_merge(tr_scene *dst, tr_scene *src);
/* The rule above on the host (no GPU needed), by the very inline function k_shadow_merge calls: n values, dst updated in
 * place.  n == 0: TR_OK; a NULL array with n > 0: TR_E_INVALID. */
int tr_shadow_merge_host(size_t n, float *dst, const float *src);

/* Screen-space ambient occlusion (upstream has only the light-space `occlusion` pipeline, shader.rs:806-960, which
 * costs a second geometry pass and replaces the picture by a grey one): the scene's CURRENT frame is darkened in place,
 * on the device, from its own z buffer -- contact shadows and creases, for a frame of any pipeline and for a merged
 * frame of two scenes (tr_scene_composite), at no geometry work.  The rule is the reference's occlusion closure
 * (shader.rs:916-944) moved from the shadow buffer to the z buffer and from world-space steps to pixel offsets:
 *   samples : ring k = 1..rings has radius r_k = (radius * k) / rings (integer division); sample i = 0..15 of a ring has
 *             the offset dx = round(r_k * sin(2 pi i / 16)), dy = round(r_k * cos(2 pi i / 16)) -- f32 products of the
 *             sixteen f32 sines, rounded half away from zero; duplicate offsets at small radii are kept and counted;
 *   pixel   : with z0 its z value (what tr_scene_read_z_f32 returns): bits(z0) == bits(f32::MIN) -- not drawn -- stays
 *             untouched.  Otherwise n = 16 * rings, inv_n = 1 / n, coef = 1, and for every ring, every sample, in order:
 *                 zq = z at (x + dx, y + dy); outside the frame or on a pixel not drawn: f32::MIN
 *                 if zq - threshold > z0:  s = min((zq - z0) / falloff, 1)  (a NaN s gives 1);  coef = coef - inv_n * s
 *             and every colour channel c becomes (coef * c + (1 - coef) * 0.0) as u8 (saturating); with TR_AO_GREY c is
 *             255 in all three channels: the reference's color_blend(white, black, coef).
 * Every f32 operation rounds once, nothing is fused; a comparison with a NaN is false, so a NaN z0 or zq occludes
 * nothing.  z, the winner words and the shadow buffer are never written. */
#define TR_AO_MAX_RADIUS 16
#define TR_AO_MAX_RINGS 4
#define TR_AO_GREY 0x1u
typedef struct tr_ao_params {
    uint32_t struct_size;   /* = sizeof(tr_ao_params) */
    uint32_t radius;        /* pixels, 1..TR_AO_MAX_RADIUS */
    uint32_t rings;         /* 1..TR_AO_MAX_RINGS, rings <= radius */
    uint32_t flags;         /* TR_AO_GREY or 0 */
    float threshold;        /* the reference's 1.0; finite, >= 0 */
    float falloff;          /* the reference's 20.0; finite, > 0 */
} tr_ao_params;
/* Shades the current frame -- what the getters mean: the last render's, a frame chosen with tr_scene_select_frame, the
 * caller's buffer after tr_scene_set_frame_buffer_device -- IN PLACE: every later consumer (the getters,
 * tr_scene_resolve, the sparse read-back, tr_scene_composite in either role, an exchange) sees the shaded frame.
 * Calling it twice shades twice.  Frames tr_scene_render holds back are submitted and the frame's depth, if it was left
 * on the chip (see TR_OPT_STORE_DEPTH), is fetched by the depth-only repeat of its pass first.  A scene that is
 * logically cleared (tr_scene_clear and nothing rendered since) has no drawn pixel: TR_OK, nothing happens.
 * Asynchronous: k_ao is enqueued on the scene's stream, a later render is ordered behind it, the result is there after
 * tr_scene_sync.  The scene's passes issued so far count as handed on, as after tr_scene_get_frame_buffer_async: a
 * frame shaded in place is not rendered again behind the caller's back (a bin overflow among them is reported,
 * TR_E_BIN_OVERFLOW).  Tiles (128 x 16) in which nothing is drawn are skipped on the fast-clear flags without reading
 * a pixel.  Without TR_AO_GREY a tile whose colour is the cleared value keeps it; with it every tile that holds a
 * drawn pixel counts as written.
 * TR_E_INVALID, nothing changed and nothing queued: a NULL argument, a wrong struct_size, a radius or ring count out of
 * range or rings > radius, a threshold that is not finite or negative, a falloff that is not finite or not positive,
 * unknown flag bits, and a BAND scene (tr_options.band_row0/1 set): the samples at a band's border lie in rows another
 * rank owns, and exchanging such a halo between ranks is deliberately not part of this call -- shade the gathered
 * frame with a scene of the whole frame, or on the host. */
int tr_scene_ambient_occlusion(tr_scene *s, const tr_ao_params *p);
/* The rule above on the host (no GPU needed), by the very inline functions k_ao calls.  z: width * height floats, index
 * x + y * width, y up (tr_scene_read_z_f32); rgb: the frame as tr_scene_get_frame_buffer returns it, row 0 = top,
 * shaded in place.  The same parameter checks; width or height 0: TR_OK, nothing to do. */
int tr_ao_host(uint32_t width, uint32_t height, const float *z /* x + y*W, y up */,
               uint8_t *rgb /* row 0 = top, in place */, const tr_ao_params *p);
/* The sample table of a call: 16 * rings pairs {dx, dy} in the rule's order (dxdy: 2 * 16 * rings values). */
int tr_ao_offsets(uint32_t radius, uint32_t rings, int8_t *dxdy);

/* Frame accumulation: the last n_frames frames of the last tr_scene_render_frames* call -- F_k, k = 0 .. n_frames - 1, is
 * the image tr_scene_get_frame_buffer would return after tr_scene_select_frame(s, k) -- averaged on the device into
 * one frame: motion blur of an animated mesh (a pose, palette, table or camera per frame) and temporal anti-aliasing
 * without reading the frames back.  With integer weights w_k and D = sum of w_k, every byte b of the frame becomes
 *     out[b] = (sum over k of w_k * F_k[b] + D / 2) / D
 * -- integer division on the stored u8 values, rounded half up, no gamma.  1 <= n_frames <= TR_ACCUMULATE_MAX_FRAMES,
 * 0 <= w_k <= 255, D >= 1; weights == NULL: every weight is 1.  A frame of weight 0 is not read.  Tiles (128 x 16) a
 * frame left empty are skipped on its fast-clear flags (three quarters of each frame of the reference's model).
 * Asynchronous, like tr_scene_resolve: k_accumulate is enqueued on the scene's stream behind the renders issued so far
 * (frames held back are submitted, a pending clear is made real), a later render is ordered behind it, the result is
 * there after tr_scene_sync.  The scene's passes issued so far count as handed on, as after
 * tr_scene_get_frame_buffer_async: a bin overflow among them is reported (TR_E_BIN_OVERFLOW), not repaired by rendering
 * again.
 * out != NULL: 3 * width * height bytes of device memory, or memory from tr_host_alloc (the kernel stores through its
 * mapped address; the buffer's sparse read-back record lapses); a pinned buffer that is too small, ordinary host memory
 * and an `out` that overlaps a frame buffer the scene has rendered into (its own, a caller's) are TR_E_INVALID.  A scene
 * of the whole frame writes every byte of `out` on every call, a band scene its band's rows and nothing else.  No frame
 * of the scene is written.
 * out == NULL: in place, into the scene's CURRENT frame, which must be one of the n_frames frames (else TR_E_INVALID).
 * Every later consumer -- the getters, tr_scene_resolve (motion blur under supersampling: accumulate, then resolve),
 * the sparse read-back, tr_scene_composite, tr_scene_band_tiles, an exchange -- sees the averaged frame; the other kept
 * frames are not written; z, the winner words and the shadow buffer are NOT touched and remain those of the selected
 * frame.  Calling it twice averages twice.
 * TR_E_INVALID with a tr_last_error text, nothing changed and nothing queued: a NULL scene, n_frames == 0,
 * n_frames > TR_ACCUMULATE_MAX_FRAMES, n_frames > tr_scene_frames_kept(s) (so anything after a plain tr_scene_render), a
 * weight above 255, every weight zero. */
#define TR_ACCUMULATE_MAX_FRAMES 32
int tr_scene_accumulate(tr_scene *s, uint32_t n_frames, const uint32_t *weights /* n_frames, or NULL */, void *out /* or NULL */);
/* The same into any host memory (3 * width * height bytes): waits for the scene first (an overflowed group is rendered
 * again before it is read), averages into a buffer of the library's, copies out and returns the frame's sticky status,
 * like tr_scene_get_resolved.  Rows outside a band scene's band are zeros. */
int tr_scene_get_accumulated(tr_scene *s, uint32_t n_frames, const uint32_t *weights, uint8_t *rgb);
/* The rule above on the host (no GPU needed), by the very inline function k_accumulate calls: frames[k] points to the
 * n_bytes bytes of F_k, out to n_bytes bytes.  The same checks of n_frames and weights; n_bytes == 0: TR_OK. */
int tr_accumulate_host(size_t n_bytes, uint32_t n_frames, const uint8_t *const *frames, const uint32_t *weights, uint8_t *out);

/* Depth of field: the scene's CURRENT frame blurred by its own z buffer, on the device -- a focused subject in front of
 * a soft background (or behind a soft foreground) for a frame of any pipeline, a merged frame (tr_scene_composite), a
 * shaded one (tr_scene_ambient_occlusion) or an averaged one (tr_scene_accumulate), without reading colour and z back
 * and without rendering jittered cameras.  The rule:
 *   circle  : the circle of confusion of a pixel with depth z (what tr_scene_read_z_f32 returns):
 *                 bits(z) == bits(f32::MIN), not drawn : coc = background_radius
 *                 otherwise : coc = min(max_radius, (((|z - focus|) - range) * scale) as u32)
 *             in f32, every operation rounded once, nothing fused; `as u32` truncates and saturates, NaN and negatives
 *             give 0.  So a NaN z gives 0 and an infinite one max_radius.
 *   weights : wt[r] = 32768 / ((2r + 1) * (2r + 1)), integer division, r = 0..8:
 *             32768, 3640, 1310, 668, 404, 270, 193, 145, 113.
 *   pixel   : with R = max_radius, the output at p = (x, y), per channel c, over the stored u8 values F:
 *                 sw = 0, sc = 0
 *                 for every q = (x + dx, y + dy), |dx| <= R, |dy| <= R, q inside the frame, max(|dx|, |dy|) <= coc(q):
 *                     sw += wt[coc(q)];  sc += wt[coc(q)] * F_q[c]
 *                 out_p[c] = (sc + sw / 2) / sw                      (u32 integer arithmetic, which cannot overflow)
 *             Scatter written as gather: a pixel spreads over the square of its own circle with a weight inverse to
 *             that square's area.  q = p always qualifies.  A q outside the frame contributes nothing.  Pixels that are
 *             not drawn take part with their stored colour (a caller's buffer may hold a backdrop there) and
 *             background_radius.
 *   TR_DOF_SHOW_COC : every pixel of the output is coc(p) * 255 / max_radius in all three channels (integer division),
 *             for choosing focus and scale by eye.
 * z, the winner words and the shadow buffer are never written. */
#define TR_DOF_MAX_RADIUS 8
#define TR_DOF_SHOW_COC 0x1u
typedef struct tr_dof_params {
    uint32_t struct_size;        /* = sizeof(tr_dof_params) = 28 */
    uint32_t max_radius;         /* pixels, 1..TR_DOF_MAX_RADIUS */
    uint32_t background_radius;  /* circle of confusion of a pixel that is not drawn, 0..max_radius */
    uint32_t flags;              /* TR_DOF_SHOW_COC or 0 */
    float focus;                 /* z in focus (the units of tr_scene_read_z_f32); finite */
    float range;                 /* half-width of the band around focus that stays sharp; finite, >= 0 */
    float scale;                 /* pixels of radius per unit of z beyond the band; finite, > 0 */
} tr_dof_params;
/* Blurs the current frame -- what the getters mean: the last render's, a frame chosen with tr_scene_select_frame, the
 * caller's buffer after tr_scene_set_frame_buffer_device.  Asynchronous and ordered like tr_scene_resolve: k_dof is
 * enqueued on the scene's stream behind the renders issued so far (frames held back are submitted, a pending clear is
 * made real, a depth left on the chip -- see TR_OPT_STORE_DEPTH -- is fetched by the depth-only repeat of the frame's
 * pass), a later render is ordered behind it, the result is there after tr_scene_sync.  The scene's passes issued so
 * far count as handed on, as after tr_scene_get_frame_buffer_async: a bin overflow among them is reported
 * (TR_E_BIN_OVERFLOW), not repaired by rendering again.  Tiles (128 x 16) whose whole 3 x 3 neighbourhood holds the
 * cleared colour are written as zeros on the fast-clear flags without reading a pixel; colour spreads into a cleared
 * tile beside a drawn one.
 * out != NULL: 3 * width * height bytes of device memory, or memory from tr_host_alloc (the kernel stores through its
 * mapped address; the buffer's sparse read-back record lapses); every byte of `out` is written on every call, the
 * scene's frame is not.
 * out == NULL: in place.  The kernel writes a frame and a set of flags of the library's, and two device-to-device copies
 * in stream order put them over the current frame and its colour-clean flags: every later consumer -- the getters,
 * tr_scene_resolve, the sparse read-back, tr_scene_composite in either role, tr_scene_band_tiles -- sees the blurred
 * frame; z, the winner words and the shadow buffer stay.  Calling it twice blurs twice.
 * A scene that is logically cleared (tr_scene_clear and nothing rendered since): out of place `out` becomes zeros
 * (hipMemsetAsync, no kernel); in place TR_OK, nothing happens.
 * TR_E_INVALID with a tr_last_error text, nothing changed and nothing queued: a NULL scene or NULL params, a wrong
 * struct_size, max_radius outside 1..TR_DOF_MAX_RADIUS, background_radius > max_radius, unknown flag bits, a focus that
 * is not finite, a range that is not finite or negative, a scale that is not finite or not positive, ordinary host
 * memory as `out`, a pinned buffer that is too small, an `out` that overlaps a frame buffer the scene has rendered into,
 * and a BAND scene (tr_options.band_row0/1 set): the taps at a band's border lie in rows another rank owns. */
int tr_scene_depth_of_field(tr_scene *s, const tr_dof_params *p, void *out /* or NULL */);
/* The same into any host memory (3 * width * height bytes): waits for the scene first (an overflowed frame is rendered
 * again before it is read), blurs into a buffer of the library's, copies out and returns the frame's sticky status,
 * like tr_scene_get_resolved.  The scene's frame stays unblurred. */
int tr_scene_get_depth_of_field(tr_scene *s, const tr_dof_params *p, uint8_t *rgb);
/* The rule above on the host (no GPU needed), by the very inline functions k_dof calls.  z: width * height floats, index
 * x + y * width, y up (tr_scene_read_z_f32); rgb: the frame as tr_scene_get_frame_buffer returns it, row 0 = top; out:
 * like rgb, and not rgb.  The same parameter checks; width or height 0: TR_OK, nothing to do. */
int tr_dof_host(uint32_t width, uint32_t height, const float *z /* x + y*W, y up */, const uint8_t *rgb /* row 0 = top */,
                uint8_t *out /* != rgb */, const tr_dof_params *p);
/* The circles of confusion of n depths under the parameters (coc: n bytes). */
int tr_dof_coc(const tr_dof_params *p, uint32_t n, const float *z, uint8_t *coc);

/* Bloom: the highlights of the scene's CURRENT frame keyed out, blurred by a fixed tent and added back, on the device --
 * bright areas (the highlights of `specular` and `phong`) bleed light.  Keyed at threshold 0 and written alone
 * (TR_BLOOM_GLOW_ONLY) the glow is the frame's plain fixed-radius tent blur: a frosted reflection, a soft impostor or a
 * glow map for tr_scene_set_texture_from_frame without a read-back.  The rule, over the stored u8 values F of the frame
 * (no gamma); a pixel outside the frame is black; R = radius:
 *   key   : m = max(F_p[0], F_p[1], F_p[2]);  B_p[c] = (m > threshold) ? F_p[c] : 0
 *   tent  : w(d) = R + 1 - |d| for |d| <= R;  S = (R + 1)^2 is the sum of the weights of one axis;  D = S^2
 *   blur  : V_p[c] = sum over |dx| <= R, |dy| <= R of w(dx) * w(dy) * B_(x + dx, y + dy)[c]
 *           (a product: a horizontal pass followed by a vertical one gives the same integers in any order; with R <= 15
 *           a horizontal sum is at most 255 * 256 and fits a u16, V at most 255 * 65536 and fits a u32 -- which is why
 *           the largest radius is 15)
 *   glow  : G_p[c] = (V_p[c] + D / 2) / D                                (integer division, rounded once)
 *   out   : min(255, F_p[c] + ((strength * G_p[c] + 128) >> 8));  TR_BLOOM_GLOW_ONLY: G_p[c], strength is not used
 * z, the winner words and the shadow buffer are never written. */
#define TR_BLOOM_MAX_RADIUS 15
#define TR_BLOOM_GLOW_ONLY 0x1u
typedef struct tr_bloom_params {
    uint32_t struct_size;   /* = sizeof(tr_bloom_params) = 20 */
    uint32_t radius;        /* 1..TR_BLOOM_MAX_RADIUS */
    uint32_t threshold;     /* 0..255; 255: nothing passes the key */
    uint32_t strength;      /* 0..1024, in 1/256 */
    uint32_t flags;         /* TR_BLOOM_GLOW_ONLY or 0 */
} tr_bloom_params;
/* Blooms the current frame -- what the getters mean: the last render's, a frame chosen with tr_scene_select_frame, the
 * caller's buffer after tr_scene_set_frame_buffer_device.  Asynchronous and ordered like tr_scene_depth_of_field: k_bloom
 * is enqueued on the scene's stream behind the renders issued so far (frames held back are submitted, a pending clear is
 * made real), a later render is ordered behind it, the result is there after tr_scene_sync.  No depth is read: a depth
 * left on the chip (see TR_OPT_STORE_DEPTH) stays there, no depth-only repeat runs and no z buffer is allocated.  The
 * scene's passes issued so far count as handed on, as after tr_scene_get_frame_buffer_async: a bin overflow among them is
 * reported (TR_E_BIN_OVERFLOW), not repaired by rendering again.  Tiles (128 x 16) whose whole 3 x 3 neighbourhood holds
 * the cleared colour are written as zeros on the fast-clear flags without reading a pixel; glow spreads into a cleared
 * tile beside a drawn one.
 * out != NULL: 3 * width * height bytes of device memory, or memory from tr_host_alloc (the kernel stores through its
 * mapped address; the buffer's sparse read-back record lapses); every byte of `out` is written on every call, the
 * scene's frame is not.
 * out == NULL: in place.  The kernel writes a frame and a set of flags of the library's (those of
 * tr_scene_depth_of_field), and two device-to-device copies in stream order put them over the current frame and its
 * colour-clean flags: every later consumer -- the getters, tr_scene_resolve, the sparse read-back, tr_scene_composite in
 * either role, tr_scene_band_tiles, tr_scene_set_texture_from_frame -- sees the bloomed frame; z, the winner words and
 * the shadow buffer stay.  Calling it twice blooms twice.
 * A scene that is logically cleared (tr_scene_clear and nothing rendered since): out of place `out` becomes zeros
 * (hipMemsetAsync, no kernel); in place TR_OK, nothing happens.
 * TR_E_INVALID with a tr_last_error text, nothing changed and nothing queued: a NULL scene or NULL params, a wrong
 * struct_size, a radius outside 1..TR_BLOOM_MAX_RADIUS, a threshold above 255, a strength above 1024, unknown flag bits,
 * ordinary host memory as `out`, a pinned buffer that is too small, an `out` that overlaps a frame buffer the scene has
 * rendered into, and a BAND scene (tr_options.band_row0/1 set): the taps at a band's border lie in rows another rank
 * owns. */
int tr_scene_bloom(tr_scene *s, const tr_bloom_params *p, void *out /* or NULL */);
/* The same into any host memory (3 * width * height bytes): waits for the scene first (an overflowed frame is rendered
 * again before it is read), blooms into a buffer of the library's, copies out and returns the frame's sticky status,
 * like tr_scene_get_resolved.  The scene's frame stays unbloomed. */
int tr_scene_get_bloom(tr_scene *s, const tr_bloom_params *p, uint8_t *rgb);
/* The rule above on the host (no GPU needed), by the very inline functions k_bloom calls.  rgb: the frame as
 * tr_scene_get_frame_buffer returns it, row 0 = top; out: like rgb, and not rgb.  The same parameter checks; width or
 * height 0: TR_OK, nothing to do. */
int tr_bloom_host(uint32_t width, uint32_t height, const uint8_t *rgb /* row 0 = top */, uint8_t *out /* != rgb */,
                  const tr_bloom_params *p);

/* Colour grading: the scene's CURRENT frame mapped through a 3-D colour lookup table on the device -- the last step of the
 * chain, which turns the linear stored picture into the one to look at: gamma or sRGB encoding, a tone curve, contrast,
 * saturation, tint, inversion, false colour, or a film grade that exists as a .cube file; one rule for every pointwise
 * colour operation.  The table holds n^3 entries of rgb8, n = 2..TR_GRADE_MAX_N, red fastest (the order of a .cube
 * file): the entry for (ir, ig, ib) is lut[((ib * n + ig) * n + ir) * 3 + c].  The rule, in integers, over the stored u8
 * channels (vr, vg, vb) of a pixel:
 *   split : per channel x: p = v_x * (n - 1);  i_x = p / 255;  f_x = p % 255   (v_x = 255: i_x = n - 1, f_x = 0)
 *           j_x = min(i_x + 1, n - 1)
 *   order : the channels by f, largest first: a, b, c   (f_a >= f_b >= f_c)
 *   walk  : V0 = entry(i_r, i_g, i_b);  V1 = V0 with channel a's index stepped to j_a;  V2 = V1 with channel b's index
 *           stepped to j_b;  V3 = entry(j_r, j_g, j_b)
 *   out   : out[ch] = ((255 - f_a) * V0[ch] + (f_a - f_b) * V1[ch] + (f_b - f_c) * V2[ch] + f_c * V3[ch] + 127) / 255
 * -- tetrahedral interpolation with weights in units of 1 / 255, which sum to 255.  There is no tie-break: where two
 * fractions are equal the vertex between them has weight 0, so any order of tied channels gives the same bytes; a
 * clamped j_x only ever carries weight 0.  (0, 0, 0) maps to entry 0 exactly ("c0" below).  An identity table
 * E(i) = round(255 i / (n - 1)) gives every byte back where n - 1 divides 255 (n = 2, 4, 6, 16, 18, ...) and is within
 * +-1 otherwise (17, 33).  z, the winner words and the shadow buffer are never written. */
#define TR_GRADE_MAX_N 33
/* The table is scene state: copied, and expanded to one word an entry on the device, once.  Synchronous: waits for the
 * scene's queued work first (frames issued so far are graded by the table they were issued under), like
 * tr_scene_set_morph_targets.  n == 0 drops the table (lut may then be NULL).  TR_E_INVALID with a tr_last_error text,
 * nothing changed: a NULL scene, n == 1, n > TR_GRADE_MAX_N, NULL lut with n > 0. */
int tr_scene_set_lut(tr_scene *s, uint32_t n, const uint8_t *lut /* 3*n*n*n, host */);
/* Grades the current frame -- what the getters mean: the last render's, a frame chosen with tr_scene_select_frame, the
 * caller's buffer after tr_scene_set_frame_buffer_device.  Asynchronous and ordered like tr_scene_bloom: k_grade is
 * enqueued on the scene's stream behind the renders issued so far (frames held back are submitted), a later render is
 * ordered behind it, the result is there after tr_scene_sync.  No depth is read: a depth left on the chip (see
 * TR_OPT_STORE_DEPTH) stays there, no depth-only repeat runs and no z buffer is allocated.  The scene's passes issued so
 * far count as handed on, as after tr_scene_get_frame_buffer_async: a bin overflow among them is reported
 * (TR_E_BIN_OVERFLOW), not repaired by rendering again.
 * Tiles (128 x 16) whose colour fast-clear flag is up are not read: they become c0.
 * out != NULL: 3 * width * height bytes of device memory, or memory from tr_host_alloc (the kernel stores through its
 * mapped address; the buffer's sparse read-back record lapses), apart from every frame buffer of the scene.  A
 * whole-frame scene writes every byte of `out` on every call; a BAND scene (tr_options.band_row0/1) writes its band's
 * rows and nothing else, as tr_scene_accumulate does.  The scene's frame is not written.
 * out == NULL: in place, by the kernel itself -- a pixel depends on itself alone, so there is no scratch frame and no
 * copy.  A flagged tile keeps its zeros and its flag where c0 is (0, 0, 0); otherwise it is stored as c0 and its flag
 * comes down.  Every later consumer -- the getters, tr_scene_resolve, the sparse read-back, tr_scene_composite in either
 * role, tr_scene_band_tiles, tr_scene_set_texture_from_frame -- sees the graded frame.  Calling it twice grades twice.
 * Band scenes are accepted either way: rows outside the band are never touched.
 * A scene that is logically cleared (tr_scene_clear and nothing rendered since): with c0 = (0, 0, 0), out of place the
 * scene's rows of `out` become zeros (hipMemsetAsync, no kernel) and in place nothing happens (TR_OK); with another c0
 * the clear is made real and the kernel runs: the frame (or `out`) holds c0 in every pixel, and a following render
 * without a clear draws over it as over a caller's backdrop.
 * TR_E_INVALID with a tr_last_error text, nothing changed and nothing queued: a NULL scene, a scene without a table,
 * ordinary host memory as `out`, a pinned buffer that is too small, an `out` that overlaps a frame buffer the scene has
 * rendered into. */
int tr_scene_grade(tr_scene *s, void *out /* or NULL */);
/* The same into any host memory (3 * width * height bytes): waits for the scene first (an overflowed frame is rendered
 * again before it is read), grades into a buffer of the library's, copies out and returns the frame's sticky status,
 * like tr_scene_get_bloom.  The scene's frame stays ungraded.  A band scene's rows outside its band read as zeros. */
int tr_scene_get_graded(tr_scene *s, uint8_t *rgb);
/* The rule above on the host (no GPU needed), by the very inline functions k_grade calls, over n_pixels packed rgb8
 * pixels in any order.  out may be rgb: the rule works in place.  The same checks of n; n_pixels 0: TR_OK, nothing to
 * do. */
int tr_grade_host(size_t n_pixels, const uint8_t *rgb, uint8_t *out /* may be rgb */, uint32_t n, const uint8_t *lut);
/* Diagnostic: k_grade's workgroups are persistent -- the launcher starts as many as the device holds at once, never
 * more than there are tiles, and each walks the tiles with the stride of the grid.  `cap` is stored on the scene: every
 * later k_grade launch of that scene starts min(cap, that number) workgroups, so that a small frame takes several rounds
 * of the walk; nothing else of the launch changes, and neither does a byte of the result.  cap == 0: no cap, the
 * default.  Returns the number of workgroups of the scene's most recent k_grade launch (0: there has been none; a call
 * that short-circuits on a logically cleared scene launches nothing), or TR_E_INVALID for a NULL scene. */
int tr_scene_debug_grade_grid(tr_scene *s, uint32_t cap);

/* Outlines: ink laid over the scene's CURRENT frame where its own z buffer has a silhouette, a depth step or a fold, on
 * the device -- a line around each model, a line where one model passes in front of another (tr_scene_composite), a line
 * along a sharp fold.  With tr_scene_grade through a posterising table it is a cel or technical-illustration look for a
 * frame of any pipeline, merged or posed, with no geometry work.  The rule, with z as tr_scene_read_z_f32 returns it
 * (index x + y * width, y up; a pixel is drawn when bits(z) != bits(f32::MIN); a larger z is nearer) and F the frame as
 * tr_scene_get_frame_buffer returns it:
 *   neighbours : the 4-neighbours of p are (x +- 1, y) and (x, y +- 1).  A neighbour outside the frame does not exist
 *             and contributes nothing: a model cut by the frame's border gets no ink there.
 *   kinds   : of a drawn pixel p with depth z0 (a pixel that is not drawn has kind 0), in f32, every operation rounded
 *             once, nothing fused, a comparison with a NaN false:
 *                 SIL = 1    : some existing neighbour is not drawn
 *                 STEP = 2   : some existing drawn neighbour q has (z0 - zq) > depth_step -- the ink sits on the nearer
 *                              side of a depth step only
 *                 CREASE = 4 : only with TR_OUTLINE_CREASES, on an axis (horizontal or vertical) whose two neighbours a
 *                              and b both exist and are drawn: |z0 - za| > depth_step is false, |z0 - zb| > depth_step is
 *                              false, and |(za + zb) - (z0 + z0)| > crease.  A plane at any tilt has second difference 0
 *                              up to rounding and gets no ink, a fold does, a depth step is left to STEP.
 *   seed    : p is a seed when its kinds are not 0.
 *   ink     : p is inked when some q inside the frame with max(|dx|, |dy|) <= radius is a seed.  Ink spreads onto pixels
 *             that are not drawn.
 *   output  : base = paper under TR_OUTLINE_ONLY, else F_p.  An inked pixel gets, per channel c,
 *                 out[c] = (ink[c] * opacity + base[c] * (256 - opacity) + 128) >> 8
 *             and any other pixel gets base.
 * z, the winner words and the shadow buffer are never written. */
#define TR_OUTLINE_MAX_RADIUS 3
#define TR_OUTLINE_CREASES 0x1u   /* also ink folds (second difference of depth) */
#define TR_OUTLINE_ONLY    0x2u   /* the base colour is `paper`, not the frame: a line drawing */
typedef struct tr_outline_params {
    uint32_t struct_size;  /* = sizeof(tr_outline_params) = 32 */
    uint32_t radius;       /* 0..TR_OUTLINE_MAX_RADIUS: ink reaches this far (Chebyshev) from a seed pixel */
    uint32_t flags;
    uint32_t opacity;      /* 0..256 */
    uint8_t  ink[4];       /* r, g, b, 0 */
    uint8_t  paper[4];     /* r, g, b, 0; read only under TR_OUTLINE_ONLY */
    float depth_step;      /* finite, >= 0, units of tr_scene_read_z_f32 */
    float crease;          /* finite, >= 0; read only under TR_OUTLINE_CREASES */
} tr_outline_params;
/* Outlines the current frame -- what the getters mean: the last render's, a frame chosen with tr_scene_select_frame, the
 * caller's buffer after tr_scene_set_frame_buffer_device.  Asynchronous and ordered like tr_scene_depth_of_field:
 * k_outline is enqueued on the scene's stream behind the renders issued so far (frames held back are submitted, a depth
 * left on the chip -- see TR_OPT_STORE_DEPTH -- is fetched by the depth-only repeat of the frame's pass), a later render
 * is ordered behind it, the result is there after tr_scene_sync.  The scene's passes issued so far count as handed on.
 * Tiles (128 x 16) whose whole 3 x 3 neighbourhood has its z fast-clear flag up hold no ink and are handled on the flags.
 * out != NULL: 3 * width * height bytes of device memory, or memory from tr_host_alloc (the kernel stores through its
 * mapped address; the buffer's sparse read-back record lapses), apart from every frame buffer of the scene; every byte
 * of `out` is written on every call, the scene's frame is not.
 * out == NULL: in place, by the kernel itself -- a pixel's output depends on the depths around it and on its own colour
 * alone, so there is no scratch frame and no copy.  A tile whose colour fast-clear flag is up and that receives no ink
 * keeps its flag and is not touched (under TR_OUTLINE_ONLY: where paper is (0, 0, 0)); ink that spreads into such a
 * tile, or a paper that is not black, stores the whole tile and lowers its flag.  Every later consumer -- the getters,
 * tr_scene_resolve, the sparse read-back, tr_scene_composite in either role, tr_scene_set_texture_from_frame -- sees
 * the outlined frame.  Calling it twice outlines twice.
 * A scene that is logically cleared (tr_scene_clear and nothing rendered since): out of place `out` becomes zeros
 * (hipMemsetAsync, no kernel), or `paper` in every pixel under TR_OUTLINE_ONLY (the clear is made real and the kernel
 * runs); in place TR_OK, nothing happens.
 * TR_E_INVALID with a tr_last_error text, nothing changed and nothing queued: a NULL scene or NULL params, a wrong
 * struct_size, radius > TR_OUTLINE_MAX_RADIUS, unknown flag bits, opacity > 256, a non-zero fourth byte of ink or paper,
 * a depth_step or crease that is not finite or is negative, ordinary host memory as `out`, a pinned buffer that is too
 * small, an `out` that overlaps a frame buffer the scene has rendered into, and a BAND scene (tr_options.band_row0/1
 * set): the neighbours at a band's border lie in rows another rank owns. */
int tr_scene_outline(tr_scene *s, const tr_outline_params *p, void *out /* or NULL */);
/* The same into any host memory (3 * width * height bytes): waits for the scene first (an overflowed frame is rendered
 * again before it is read), outlines into a buffer of the library's, copies out and returns the frame's sticky status,
 * like tr_scene_get_depth_of_field.  The scene's frame stays as it is. */
int tr_scene_get_outlined(tr_scene *s, const tr_outline_params *p, uint8_t *rgb);
/* The rule above on the host (no GPU needed), by the very inline functions k_outline calls.  z: width * height floats,
 * index x + y * width, y up; rgb: row 0 = top; out: like rgb, and may be rgb.  The same parameter checks; width or height
 * 0: TR_OK, nothing to do. */
int tr_outline_host(uint32_t width, uint32_t height, const float *z /* x + y*W, y up */, const uint8_t *rgb /* row 0 = top */,
                    uint8_t *out /* may be rgb */, const tr_outline_params *p);
/* The kind bits (SIL 1, STEP 2, CREASE 4) of every pixel under the parameters, in z's orientation (kinds: width * height
 * bytes) -- for choosing depth_step and crease. */
int tr_outline_kinds(uint32_t width, uint32_t height, const float *z, const tr_outline_params *p, uint8_t *kinds);

/* Edge anti-aliasing: the stair-steps of the scene's CURRENT frame smoothed on the device, at the frame's own size and
 * without geometry -- a luma-driven edge filter of the FXAA family, in integers on the stored bytes.  It works on any
 * frame: rendered, composited, graded, inked by tr_scene_outline.  The rule, in the orientation of
 * tr_scene_get_frame_buffer (row 0 = top, y grows downwards; N is (x, y - 1), S (x, y + 1), W (x - 1, y), E (x + 1, y)):
 * F(x, y) is the stored rgb8 and L(x, y) = (54 R + 183 G + 19 B + 128) >> 8 its luma, the Y of tr_frame_stats.  A
 * coordinate outside the frame is clamped to it, x and y each on its own: the border pixel repeats.  For every pixel p:
 *   1 contrast : M, N, S, W, E the lumas of p and its four neighbours, lo / hi their min / max, range = hi - lo.
 *                range < max(contrast_min, (hi * contrast_rel + 128) >> 8), or range == 0: off = 0, p is kept.
 *   2 direction: EH = |NW + SW - 2 W| + 2 |N + S - 2 M| + |NE + SE - 2 E|
 *                EV = |NW + NE - 2 N| + 2 |W + E - 2 M| + |SW + SE - 2 S|;  the edge is horizontal when EH >= EV.
 *   3 sides    : horizontal: A = N, B = S, t = (1, 0); vertical: A = W, B = E, t = (0, 1).  gA = |A - M|, gB = |B - M|;
 *                the side is A when gA >= gB, else B; g = max(gA, gB); C the chosen neighbour's luma, n the unit step
 *                from p to it; mid2 = M + C.
 *   4 search   : for s in {-1, +1}, each on its own: k = 1 .. search, q = p + s k t, d2 = L(q) + L(q + n) - mid2, stop at
 *                the first k with 2 |d2| >= g.  dist_s = that k, or `search` when none stopped; end_s = the last d2
 *                evaluated.
 *   5 edge     : span = dist_- + dist_+; the near end is the - end when dist_- < dist_+, else the + end, with `near` its
 *                distance and `end` its d2.  good = (end < 0) != (2 M - mid2 < 0).
 *                off_e = good ? ((span - 2 near) * 128 + span / 2) / span : 0            (floor divisions; 0..128)
 *   6 sub-pixel: a = |2 (N + S + W + E) + NW + NE + SW + SE - 12 M|;  tq = min(256, (a * 256) / (12 * range))
 *                sm = (tq * tq * (768 - 2 tq)) >> 16;  off_s = (((sm * sm) >> 8) * subpixel) >> 8          (0..256)
 *   7 output   : off = max(off_e, off_s); out[c] = (F_p[c] * (256 - off) + F_(p + n)[c] * off + 128) >> 8, p + n clamped
 *                like every coordinate.  Under TR_AA_SHOW_BLEND all three channels are min(255, off) instead (0 for a
 *                kept pixel): what the filter found, a diagnostic like TR_DOF_SHOW_COC.
 * z, the winner words and the shadow buffer are neither read nor written. */
#define TR_AA_MAX_SEARCH 8
#define TR_AA_SHOW_BLEND 0x1u
typedef struct tr_aa_params {
    uint32_t struct_size;   /* = sizeof(tr_aa_params) = 24 */
    uint32_t contrast_min;  /* 0..255: a pixel whose local luma range is below it is kept */
    uint32_t contrast_rel;  /* 0..256: ... or below this many 256ths of the brightest of the five lumas */
    uint32_t search;        /* 1..TR_AA_MAX_SEARCH: how far along the edge its ends are looked for */
    uint32_t subpixel;      /* 0..256: the weight of the sub-pixel term (0: edges only) */
    uint32_t flags;
} tr_aa_params;
/* Filters the current frame -- what the getters mean.  Asynchronous and ordered like tr_scene_bloom: k_aa is enqueued on
 * the scene's stream behind the renders issued so far (frames held back are submitted; no depth is read, so a depth left
 * on the chip stays there), a later render is ordered behind it, the result is there after tr_scene_sync.  The scene's
 * passes issued so far count as handed on.  Tiles (128 x 16) whose whole 3 x 3 neighbourhood has its colour fast-clear
 * flag up are black, stay black and are handled on the flags.
 * out != NULL: 3 * width * height bytes of device memory, or memory from tr_host_alloc (the kernel stores through its
 * mapped address; the buffer's sparse read-back record lapses), apart from every frame buffer of the scene; every byte
 * of `out` is written on every call, the scene's frame is not.
 * out == NULL: in place -- through a scratch frame of the scene's and a device-to-device copy, because a pixel reads its
 * neighbours.  A tile whose colour flag is up keeps it unless colour came in from a neighbour's edge (some byte of its
 * output is not zero): then its flag is lowered.  Every later consumer sees the filtered frame; calling it twice
 * filters twice.
 * A scene that is logically cleared (tr_scene_clear and nothing rendered since) is black and stays black: out of place
 * `out` becomes zeros (hipMemsetAsync, no kernel); in place TR_OK, nothing happens.
 * TR_E_INVALID with a tr_last_error text, nothing changed and nothing queued: a NULL scene or NULL params, a wrong
 * struct_size, contrast_min > 255, contrast_rel > 256, search outside 1..TR_AA_MAX_SEARCH, subpixel > 256, unknown flag
 * bits, ordinary host memory as `out`, a pinned buffer that is too small, an `out` that overlaps a frame buffer the
 * scene has rendered into, and a BAND scene (tr_options.band_row0/1 set): the taps at a band's border lie in rows
 * another rank owns. */
int tr_scene_antialias(tr_scene *s, const tr_aa_params *p, void *out /* or NULL */);
/* The same into any host memory (3 * width * height bytes): waits for the scene first, filters into a buffer of the
 * library's, copies out and returns the frame's sticky status, like tr_scene_get_bloom.  The scene's frame stays. */
int tr_scene_get_antialiased(tr_scene *s, const tr_aa_params *p, uint8_t *rgb);
/* The rule above on the host (no GPU needed), by the very inline functions k_aa calls.  rgb and out: 3 * width * height
 * bytes, row 0 = top; out must not be rgb.  The same parameter checks; width or height 0: TR_OK, nothing to do. */
int tr_aa_host(uint32_t width, uint32_t height, const uint8_t *rgb, uint8_t *out /* != rgb */, const tr_aa_params *p);
/* The rule's two floor divisions as device and host compute them, for checking them exhaustively: out[i] = the edge
 * term of span a[i] (2..16) and near b[i] (1..a[i] / 2) when which == 0, tq of a = a[i] (0..3060) and range b[i] (1..255)
 * when which == 1.  TR_E_INVALID for another `which`, a NULL pointer with n > 0, or a pair outside those ranges. */
int tr_aa_quotients(uint32_t which, uint32_t n, const uint32_t *a, const uint32_t *b, uint32_t *out);

/* Resize: the scene's CURRENT frame, W x H, scaled on the device to any width x height -- 1920 x 1080 from 4096^2, a
 * thumbnail, a x 1.5 preview, a half-size render shown at full size -- by a separable filter with integer weights, the
 * last step of the chain (render, composite, ..., antialias, RESIZE, read back or tr_scene_set_texture_device).  F is
 * the image tr_scene_get_frame_buffer would return and `out` has its orientation (row 0 = top), tightly packed rgb8.
 * The axes are independent (the two ratios may differ).  For ONE axis with N source and M output samples, output index X
 * gets raw integer taps o[x] over the source indices x in [0, N):
 *   TR_RESIZE_AREA      o[x] = max(0, min((x + 1) M, (X + 1) N) - max(x M, X N)): the overlap of the two pixels'
 *                       intervals in units of 1 / (N M);
 *   TR_RESIZE_BILINEAR  a triangle whose support grows with the ratio when minifying: S = 2 max(M, N), C = (2 X + 1) N,
 *                       o[x] = max(0, S - |(2 x + 1) M - C|); taps that would fall outside [0, N) are dropped, not
 *                       clamped, and the normalisation makes up for them.
 * The taps with o[x] > 0 form one run x0 .. x0 + n - 1 and their weights sum to exactly 4096 by cumulative rounding:
 * O = sum of o, cum_k = o[x0] + .. + o[x0 + k], c_k = (4096 cum_k + O / 2) / O (integer division), w_k = c_k - c_(k-1)
 * with c_(-1) = 0; a weight may come out 0 and is kept.  Then
 *     out[Y][X][c] = ( sum_j wy[Y][j] * ( sum_k wx[X][k] * F[y0(Y) + j][x0(X) + k][c] ) + 2^23 ) >> 24
 * with the inner sum unrounded; everything fits 32 bits.  So: the same size is a copy, a constant frame stays constant,
 * and TR_RESIZE_AREA at W / f x H / f, f = 2, 4, 8, equals tr_scene_resolve(f) in every byte.  No gamma.
 * Limits: ceil(N / 8) <= M <= 8192 on each axis -- a minification beyond 8 is refused, a magnification is bounded by the
 * size alone --, within which a run has at most TR_RESIZE_MAX_TAPS taps; filter is one of the two; flags must be 0. */
#define TR_RESIZE_AREA 0u
#define TR_RESIZE_BILINEAR 1u
#define TR_RESIZE_MAX_TAPS 16
typedef struct tr_resize_params {
    uint32_t width, height; /* of the output, each 1..8192 and at least an eighth of the frame's, rounded up */
    uint32_t filter;        /* TR_RESIZE_AREA or TR_RESIZE_BILINEAR */
    uint32_t flags;         /* 0 */
} tr_resize_params;
/* Resizes the current frame -- what the getters mean: the last render's, a frame chosen with tr_scene_select_frame, the
 * caller's buffer after tr_scene_set_frame_buffer_device.  Asynchronous and ordered like tr_scene_resolve: frames held
 * back are submitted, a pending clear is made real, k_resize is enqueued on the scene's stream behind the renders issued
 * so far (no depth is read, so a depth left on the chip stays there), a later render is ordered behind it, the result is
 * there after tr_scene_sync.  The scene's passes issued so far count as handed on.  The weights are computed on the
 * host; their tables are kept on the scene for the last (width, height, filter) and uploaded again, in stream order,
 * only when that changes.  An output tile whose whole source footprint has its colour fast-clear flags up is stored as
 * zeros without a load.
 * out: 3 * width * height bytes of device memory, or memory from tr_host_alloc (the kernel stores through its mapped
 * address; the buffer's sparse read-back record lapses); every byte of it is written on every call.  The output is no
 * frame of the scene: there is no in-place form and out == NULL is refused.
 * A scene that is logically cleared (tr_scene_clear and nothing rendered since) is black at every size: `out` becomes
 * zeros (hipMemsetAsync, no kernel).
 * TR_E_INVALID with a tr_last_error text that names the call, nothing changed and nothing queued: a NULL scene, params
 * or out, flags != 0, an unknown filter, a width or height outside the limits above, ordinary host memory as `out`, a
 * pinned buffer that is too small, and a BAND scene (tr_options.band_row0/1 set): the taps at a band's border lie in
 * rows another rank owns. */
int tr_scene_resize(tr_scene *s, const tr_resize_params *p, void *out);
/* The same into any host memory (3 * p->width * p->height bytes): waits for the scene first, resizes into a buffer of
 * the library's, copies out and returns the frame's sticky status, like tr_scene_get_resolved.  A cleared scene gives
 * zeros. */
int tr_scene_get_resized(tr_scene *s, const tr_resize_params *p, uint8_t *rgb);
/* The rule above on the host (no GPU needed), through the tables k_resize is fed.  rgb: 3 * width * height bytes, out:
 * 3 * p->width * p->height bytes, both row 0 = top; out must not be rgb.  The same parameter checks, with width and
 * height (each >= 1) in the frame's place. */
int tr_resize_host(uint32_t width, uint32_t height, const uint8_t *rgb, const tr_resize_params *p, uint8_t *out /* != rgb */);
/* The tables of one axis as the kernel is fed them, for checking them against the rule: for every output index X the
 * first source index of its run, the run's length (1..TR_RESIZE_MAX_TAPS) and its weights, zeros beyond the length.
 * TR_E_INVALID for an unknown filter, an n_dst outside ceil(n_src / 8)..8192, n_src == 0 or a NULL pointer. */
int tr_resize_taps(uint32_t filter, uint32_t n_src, uint32_t n_dst, uint16_t *first /* n_dst */, uint16_t *count /* n_dst */,
                   uint16_t *weights /* n_dst * TR_RESIZE_MAX_TAPS, zero-padded */);

/* Warp: the scene's CURRENT frame, W x H, resampled on the device through a coarse grid of source coordinates -- one
 * grid and one kernel for every geometric operation: rotation, flip, lens distortion (Brown-Conrady), keystone, crop and
 * zoom, stabilisation, separated colour channels; each is a different grid built on the host.  In the chain it stands
 * after antialias and before resize.  F is the image tr_scene_get_frame_buffer would return; the output is W' x H', each
 * 1..8192, with F's orientation (row 0 = top), tightly packed rgb8.
 * Grid.  Nodes are TR_WARP_CELL = 16 output pixels apart: gw = (W' + 15) / 16 + 1 by gh = (H' + 15) / 16 + 1 nodes,
 * row-major, each a pair of int32_t (sx, sy) in units of 1/256 source pixel.  256 * x means exactly source sample x (a
 * sample-index convention, no half-pixel offset).  Every node value lies in [-2^22, 2^22]; others are refused.
 * Per output pixel (X, Y): gx = X >> 4, fx = X & 15, gy = Y >> 4, fy = Y & 15, and for both coordinates
 *     s = ((16-fx)(16-fy) n00 + fx (16-fy) n10 + (16-fx) fy n01 + fx fy n11 + 128) >> 8    (arithmetic shift: floor; i32)
 * over the cell's nodes n00 = (gx, gy), n10 = (gx + 1, gy), n01 = (gx, gy + 1), n11 = (gx + 1, gy + 1).
 * Sample.  ix = sx >> 8 (floor), ax = sx & 255, likewise iy, ay;
 *     out[c] = ((256-ax)(256-ay) T(ix,iy) + ax (256-ay) T(ix+1,iy) + (256-ax) ay T(ix,iy+1) + ax ay T(ix+1,iy+1) + 2^15) >> 16
 * in u32.  Edge: under TR_WARP_BORDER T is border[c] for a texel outside [0, W) x [0, H); under TR_WARP_CLAMP each texel
 * index is clamped to the image.  A texel of weight 0 contributes nothing either way.
 * TR_WARP_PER_CHANNEL (flags): the scene's grid must be three grids -- r, g, b, gw * gh nodes apart -- and each channel is
 * sampled at its own coordinate; without the flag it must be one.
 * So: the identity grid (node = 256 * 16 * (gx, gy)) at W' x H' = W x H is a copy, sx = 256 * (W - 1 - 16 gx) is a
 * horizontal flip, a quarter turn is exact, a whole-pixel translation is a shifted copy with border, sx = 128 X doubles
 * the width with (a + b + 1) >> 1 midpoints, and a constant frame stays constant under TR_WARP_CLAMP.
 * The filter is 2 x 2 and no wider: a grid that minifies strongly ALIASES -- shrink with tr_scene_resize. */
#define TR_WARP_CELL 16
#define TR_WARP_BORDER 0u
#define TR_WARP_CLAMP 1u
#define TR_WARP_PER_CHANNEL 1u
typedef struct tr_warp_params {
    uint32_t edge;     /* TR_WARP_BORDER or TR_WARP_CLAMP */
    uint8_t border[3]; /* r, g, b of a texel outside the image under TR_WARP_BORDER */
    uint8_t pad;       /* 0 */
    uint32_t flags;    /* 0 or TR_WARP_PER_CHANNEL */
} tr_warp_params;
/* The scene's grid: the output is width x height (each 1..8192) and `grid` holds n_grids (1, or 3 for
 * TR_WARP_PER_CHANNEL) grids of gw * gh node pairs.  The nodes are checked and copied before the call returns, then
 * uploaded in stream order and kept on the scene until the next call: work already issued keeps the old grid.
 * TR_E_INVALID with a text that names the call, nothing changed: a NULL scene or grid, a size outside 1..8192, n_grids
 * not 1 or 3, a node value outside [-2^22, 2^22]. */
int tr_scene_set_warp(tr_scene *s, uint32_t width, uint32_t height, uint32_t n_grids, const int32_t *grid);
/* Warps the current frame -- what the getters mean: the last render's, a frame chosen with tr_scene_select_frame, the
 * caller's buffer after tr_scene_set_frame_buffer_device -- through the scene's grid.  Asynchronous and ordered like
 * tr_scene_bloom: frames held back are submitted, a pending clear is made real, k_warp is enqueued on the scene's stream
 * behind the renders issued so far (no depth is read, so a depth left on the chip stays there), a later render is ordered
 * behind it, the result is there after tr_scene_sync.  The scene's passes issued so far count as handed on.
 * out: 3 * W' * H' bytes (the grid's size) of device memory, or memory from tr_host_alloc (the kernel stores through its
 * mapped address; the buffer's sparse read-back record lapses); every byte of it is written; it must not overlap a frame
 * buffer of the scene.  out == NULL: IN PLACE, allowed only when the grid's size is the frame's: the warped frame
 * replaces the current one (through a scratch frame of the scene's) with its colour fast-clear flags, and every later
 * consumer sees it.  An output tile whose whole source footprint has its colour fast-clear flags up is stored as zeros
 * without a load where the rule gives black there; a texel behind a raised flag is never loaded.
 * A scene that is logically cleared (tr_scene_clear and nothing rendered since) maps to black under TR_WARP_CLAMP or a
 * border of 0: `out` becomes zeros (hipMemsetAsync, no kernel), and in place nothing happens.  With another border the
 * clear is made real and the kernel runs.
 * TR_E_INVALID with a tr_last_error text that names the call, nothing changed and nothing queued: a NULL scene or
 * params, an unknown edge, pad != 0, unknown flags; no grid set (tr_scene_set_warp), a grid count that does not match
 * TR_WARP_PER_CHANNEL, a BAND scene (tr_options.band_row0/1 set); ordinary host memory as `out`, a pinned buffer that
 * is too small, an `out` that overlaps a frame, out == NULL with a grid of another size than the frame's. */
int tr_scene_warp(tr_scene *s, const tr_warp_params *p, void *out);
/* The same into any host memory (3 * W' * H' bytes): waits for the scene first, warps into a buffer of the library's,
 * copies out and returns the frame's sticky status, like tr_scene_get_bloom. */
int tr_scene_get_warped(tr_scene *s, const tr_warp_params *p, uint8_t *rgb);
/* The rule above on the host (no GPU needed).  rgb: 3 * width * height bytes, out: 3 * out_width * out_height bytes,
 * both row 0 = top; out must not be rgb.  The same parameter and grid checks, with width and height (each >= 1) in the
 * frame's place. */
int tr_warp_host(uint32_t width, uint32_t height, const uint8_t *rgb, uint32_t out_width, uint32_t out_height, uint32_t n_grids,
                 const int32_t *grid, const tr_warp_params *p, uint8_t *out /* != rgb */);

/* Convolve: the scene's CURRENT frame filtered on the device through a kernel of integer weights -- one kernel
 * (k_convolve) for every linear neighbourhood filter: Gaussian and box blur, sharpen and unsharp mask, emboss, Laplacian,
 * Sobel, directional blur.  F is the frame as tr_scene_get_frame_buffer returns it: rgb8, row 0 = top, y grows downward.
 * kw x kh taps, both odd; w(i, j) is the weight of column i from the left, row j from the top:
 *   general   : w(i, j) = weights[j * kw + i], kw and kh 1..9
 *   separable : row = weights[0 .. kw), col = weights[kw .. kw + kh), w(i, j) = row[i] * col[j], kw and kh 1..31
 *   sum   : acc[c] = sum over j < kh, i < kw of w(i, j) * F(x + i - kw / 2, y + j - kh / 2)[c]    (correlation: no flip)
 *           a tap outside the image is border[c] under TR_CONVOLVE_BORDER; under TR_CONVOLVE_CLAMP its index is clamped
 *           per axis
 *   scale : v = (acc + rnd) >> shift, an arithmetic shift, rnd = shift ? 1 << (shift - 1) : 0;  TR_CONVOLVE_ABS: v = |v|
 *   out   : clamp(v + bias, 0, 255)
 *           TR_CONVOLVE_UNSHARP: v = clamp(v, 0, 255), out = clamp(F + ((amount * (F - v) + 128) >> 8), 0, 255) with an
 *           arithmetic shift; bias must be 0 and TR_CONVOLVE_ABS is refused: sharpening at any radius up to 15 is one
 *           separable call
 * Bounds: A = sum |w| (general) or sum |row| * sum |col| (separable) must not exceed 2^22 -- then 255 A + 2^21 < 2^31 and an
 * int32 holds every sum; no int16 kernel of the general form is refused on it (81 * 32767 < 2^22).  Separable: sum |row|
 * must not exceed 2^15 either.  The separable form is DEFINED as the 2-D sum of the outer product; everything is integer,
 * so the device equals tr_convolve_host in every byte.  1 x 1 with w = 1 and shift 0 is a copy; a single tap of 1 off
 * centre is a shifted copy; a separable kernel of at most 9 x 9 equals its outer product through the general form; the
 * tent row = col = [1 .. R + 1 .. 1] with shift = 4 log2(R + 1) and a border of 0 is tr_scene_bloom's glow at threshold 0
 * for R = 1, 3, 7, 15. */
#define TR_CONVOLVE_SEPARABLE 1u
#define TR_CONVOLVE_ABS 2u
#define TR_CONVOLVE_UNSHARP 4u
#define TR_CONVOLVE_BORDER 0u
#define TR_CONVOLVE_CLAMP 1u
typedef struct tr_convolve_params {
    uint32_t struct_size;   /* = sizeof(tr_convolve_params) = 200 */
    uint32_t kw, kh;        /* odd; general form 1..9 each, TR_CONVOLVE_SEPARABLE 1..31 each */
    uint32_t flags;         /* TR_CONVOLVE_SEPARABLE | TR_CONVOLVE_ABS | TR_CONVOLVE_UNSHARP */
    uint32_t shift;         /* 0..22 */
    int32_t bias;           /* -255..255 */
    uint32_t amount;        /* 0..1024 in 1/256; read under TR_CONVOLVE_UNSHARP only, else must be 0 */
    uint32_t edge;          /* TR_CONVOLVE_BORDER or TR_CONVOLVE_CLAMP */
    uint8_t border[3];      /* r, g, b of a tap outside the image under TR_CONVOLVE_BORDER */
    uint8_t pad;            /* 0 */
    int16_t weights[82];    /* see above; entries behind the last one used are not read */
} tr_convolve_params;
/* Filters the current frame -- what the getters mean.  Asynchronous and ordered like tr_scene_bloom: frames held back are
 * submitted, a pending clear is made real, k_convolve is enqueued on the scene's stream.  No depth is read, so a depth
 * left on the chip stays there.  out: 3 * W * H bytes of device memory or of memory from tr_host_alloc, apart from every
 * frame buffer of the scene; every byte is written and the scene's frame stays.  out == NULL: IN PLACE -- every later
 * consumer sees the filtered frame, the colour fast-clear flags follow (a tile is flagged only where it is zeros in
 * every byte), z, the winner words and the shadow buffer stay; calling it twice filters twice.  A tile whose 3 x 3
 * neighbourhood is flagged clean is not read: it becomes clamp(bias) (0 under TR_CONVOLVE_UNSHARP) where no border
 * colour reaches it.  A scene that is logically cleared maps to black where the rule gives black -- clamp(bias) == 0 and
 * (TR_CONVOLVE_CLAMP or a border of 0): zeros out of place, nothing in place, no kernel; otherwise the clear is made real
 * and the kernel runs.
 * TR_E_INVALID, each text opening with the call's name: a null scene or params, a wrong struct_size, unknown flags, an
 * even or out-of-range kw or kh, a shift above 22, a bias outside -255..255, an amount above 1024 or non-zero without
 * TR_CONVOLVE_UNSHARP, an unknown edge, pad != 0, weights beyond either bound, TR_CONVOLVE_UNSHARP with TR_CONVOLVE_ABS or
 * a bias; a BAND scene (tr_options.band_row0/1 set: the taps at a band's border lie in another rank's rows); ordinary
 * host memory as `out`, a pinned buffer that is too small, an `out` that overlaps a frame buffer of the scene. */
int tr_scene_convolve(tr_scene *s, const tr_convolve_params *p, void *out /* or NULL */);
/* The same into any host memory (3 * W * H bytes): waits for the scene first, filters into a buffer of the library's,
 * copies out and returns the frame's sticky status, like tr_scene_get_bloom.  The scene's frame stays. */
int tr_scene_get_convolved(tr_scene *s, const tr_convolve_params *p, uint8_t *rgb);
/* The rule above on the host (no GPU needed), by the very inline functions k_convolve calls.  rgb and out: 3 * width *
 * height bytes, row 0 = top; out must not be rgb.  The same parameter checks; a width or height of 0 returns TR_OK. */
int tr_convolve_host(uint32_t width, uint32_t height, const uint8_t *rgb /* row 0 = top */, uint8_t *out /* != rgb */,
                     const tr_convolve_params *p);

/* Rank: the scene's CURRENT frame through an order-statistic neighbourhood filter on the device -- one kernel (k_rank)
 * for median, minimum (erode), maximum (dilate) and what is built from them: open, close, morphological gradient,
 * despeckle.  No stack of convolutions expresses these.
 * Input.  F is the frame as tr_scene_get_frame_buffer returns it: rgb8, row 0 at the top.
 * Footprint.  A set of taps inside a kw x kh box; kw and kh are odd and each is 1..15.  It is given as rows[15] of
 * uint16_t: bit i of rows[j] set means that column i from the left, row j from the TOP, is a tap.  Bits at or beyond kw,
 * and rows at or beyond kh, must be 0.  n, the number of taps, must be at least 1.  Rows or columns inside the box may be
 * empty, and the centre need not be a tap.  Tap (i, j) of pixel (x, y) reads F(x + i - kw / 2, y + j - kh / 2).
 * Edge handling.  Under TR_RANK_BORDER a tap outside the image is border[c]; under TR_RANK_CLAMP its index is clamped
 * per axis.
 * Ranking.  For each channel independently, sort the n tap values in ascending order; v(k) is element k, 0-based.
 * Operations (op):
 *   TR_RANK_VALUE         v(rank).  Rank 0 is erode, rank n - 1 is dilate, and the middle rank is the median.
 *   TR_RANK_RANGE         v(rank2) - v(rank).  The morphological gradient is this at ranks 0 and n - 1.
 *   TR_RANK_MID           (v(rank) + v(rank2) + 1) >> 1
 *   TR_RANK_CLAMP_CENTRE  min(max(F(x, y), v(rank)), v(rank2)): conservative despeckle -- a pixel is changed only if it
 *                         lies outside the rank interval of its neighbourhood.
 * rank <= rank2 <= n - 1; under TR_RANK_VALUE rank2 must be 0.
 * Order statistics are exact, so the device equals tr_rank_host in every byte.  What follows from the rule: a one-tap
 * footprint under TR_RANK_VALUE is a copy -- off centre a shifted copy, with the border colour entering; a constant frame
 * under TR_RANK_CLAMP stays constant, and its TR_RANK_RANGE is 0; rank k of F equals 255 - rank (n - 1 - k) of (255 - F)
 * with the border complemented; TR_RANK_VALUE at rank 0 or n - 1 over a full kw x kh rectangle equals the kw x 1 call
 * followed by the 1 x kh call, under either edge mode. */
#define TR_RANK_VALUE 0u
#define TR_RANK_RANGE 1u
#define TR_RANK_MID 2u
#define TR_RANK_CLAMP_CENTRE 3u
#define TR_RANK_BORDER 0u
#define TR_RANK_CLAMP 1u
typedef struct tr_rank_params {
    uint32_t struct_size;   /* = sizeof(tr_rank_params) = 64 */
    uint32_t kw, kh;        /* odd, 1..15 each */
    uint32_t op;            /* TR_RANK_VALUE, TR_RANK_RANGE, TR_RANK_MID or TR_RANK_CLAMP_CENTRE */
    uint32_t rank, rank2;   /* 0-based; rank2 is 0 under TR_RANK_VALUE, else rank <= rank2 <= n - 1 */
    uint32_t edge;          /* TR_RANK_BORDER or TR_RANK_CLAMP */
    uint8_t border[3];      /* r, g, b of a tap outside the image under TR_RANK_BORDER */
    uint8_t pad;            /* 0 */
    uint16_t rows[15];      /* bit i of rows[j]: column i from the left, row j from the top is a tap */
    uint16_t pad2;          /* 0 */
} tr_rank_params;
/* Filters the current frame -- what the getters mean.  Asynchronous and ordered like tr_scene_convolve: frames held back
 * are submitted, a pending clear is made real, k_rank is enqueued on the scene's stream.  No depth is read, so a depth
 * left on the chip stays there.  out: 3 * W * H bytes of device memory or of memory from tr_host_alloc, apart from every
 * frame buffer of the scene; every byte is written and the scene's frame stays.  out == NULL: IN PLACE, through the
 * scene's scratch frame (a tap reads neighbours) -- every later consumer sees the filtered frame, the colour fast-clear
 * flags follow (a tile is flagged only where it is zeros in every byte), z, the winner words and the shadow buffer stay;
 * calling it twice filters twice, so open is erode then dilate.  A tile whose existing 3 x 3 neighbourhood is flagged
 * clean, with no non-zero border colour in reach (TR_RANK_CLAMP, a border of 0, or a halo inside the image), is 0 under
 * every op: it is stored without a load.  A texel behind a raised flag counts as zeros and is never loaded.  A scene that
 * is logically cleared under TR_RANK_CLAMP or a border of 0: zeros out of place, nothing in place, no kernel; otherwise
 * the clear is made real and the kernel runs.
 * TR_E_INVALID, each text opening with the call's name: a null scene or params, a wrong struct_size, an even or
 * out-of-range kw or kh, footprint bits outside the box, an empty footprint, an unknown op or edge, pad or pad2 != 0, a
 * rank or rank2 >= n, rank > rank2, a non-zero rank2 under TR_RANK_VALUE; a BAND scene (tr_options.band_row0/1 set: the
 * taps at a band's border lie in another rank's rows); ordinary host memory as `out`, a pinned buffer that is too small,
 * an `out` that overlaps a frame buffer of the scene.  The parameters are checked first, then the band, then `out`. */
int tr_scene_rank(tr_scene *s, const tr_rank_params *p, void *out /* or NULL */);
/* The same into any host memory (3 * W * H bytes): waits for the scene first, filters into a buffer of the library's,
 * copies out and returns the frame's sticky status, like tr_scene_get_convolved.  The scene's frame stays. */
int tr_scene_get_ranked(tr_scene *s, const tr_rank_params *p, uint8_t *rgb);
/* The rule above on the host (no GPU needed), by the inline functions k_rank shares.  rgb and out: 3 * width * height
 * bytes, row 0 = top; out must not be rgb.  The same parameter checks; a width or height of 0 returns TR_OK. */
int tr_rank_host(uint32_t width, uint32_t height, const uint8_t *rgb /* row 0 = top */, uint8_t *out /* != rgb */,
                 const tr_rank_params *p);

/* Bilateral: the scene's CURRENT frame through an edge-preserving smoothing filter on the device -- one kernel
 * (k_bilateral): a weighted mean over a window whose weights fall with a tap's difference from the centre pixel, in
 * colour or in depth.  The third neighbourhood family beside the linear one (convolve) and the order statistics (rank);
 * no stack of those expresses it.  Guided by depth it is the "joint" or "cross" bilateral blur that takes the grain out
 * of ambient occlusion and of shadow borders without bleeding across silhouettes; guided by colour and followed by a
 * posterising grade table and an outline it is the usual toon look.
 * Input.  F is the frame as tr_scene_get_frame_buffer returns it: rgb8, row 0 at the top.  z is the depth as tr_dof_host
 * takes it: index x + y*W, y up; a pixel is not drawn when bits(z) == bits(f32::MIN).
 * Window.  kw x kh, each odd and 1..15.  spatial[j*kw + i] is a u8 weight for column i from the left and row j from the
 * TOP; a tap with spatial weight 0 is no tap.  Bytes of spatial at index kw*kh and beyond must be 0, and at least one
 * weight must be non-zero.  Tap (i, j) of pixel (x, y) reads position (x + i - kw/2, y + j - kh/2).
 * Edge handling.  Under TR_BILATERAL_BORDER a tap outside the image has colour border[c] and depth f32::MIN; under
 * TR_BILATERAL_CLAMP its index is clamped per axis, for colour and depth alike.
 * Distance d of a tap T from the centre C, 0..255:
 *   TR_BILATERAL_GUIDE_COLOUR  d = max(|Tr-Cr|, |Tg-Cg|, |Tb-Cb|)
 *   TR_BILATERAL_GUIDE_DEPTH   t = fl(|fl(zT - zC)| * depth_scale), every f32 operation rounded once;
 *                              d = t < 255.0f ? (uint32_t)t : 255.  A NaN or an infinity therefore gives 255, two
 *                              undrawn pixels give 0.  depth_scale must be finite and >= 0.
 * Weight and sums.  w = spatial * range[d], range a table of 256 u8 entries, so w <= 65025.  S is the sum of w over the
 * taps, A_c the sum of w * T_c.  Output channel: S == 0 ? C_c : (A_c + S/2) / S, an integer division.
 * Bounds.  S <= 225 * 65025 < 2^24, and A_c + S/2 <= 225 * 65025 * 255 + 7,315,312 = 3,738,124,687 < 2^32: u32
 * accumulators suffice and each product fits a 24-bit multiply.
 * Every step is an integer or a single-rounded f32 operation, so the device equals tr_bilateral_host in every byte.  What
 * follows from the rule: a window whose only weight is the centre's, or an all-zero range table, is the identity; an
 * all-255 range table is a plain weighted mean; range[d] = 255 for d <= cutoff and 0 beyond averages exactly the taps
 * within the cutoff of the centre. */
#define TR_BILATERAL_GUIDE_COLOUR 0u
#define TR_BILATERAL_GUIDE_DEPTH 1u
#define TR_BILATERAL_BORDER 0u
#define TR_BILATERAL_CLAMP 1u
typedef struct tr_bilateral_params {
    uint32_t struct_size;   /* = sizeof(tr_bilateral_params) = 512 */
    uint32_t kw, kh;        /* odd, 1..15 each */
    uint32_t guide;         /* TR_BILATERAL_GUIDE_COLOUR or TR_BILATERAL_GUIDE_DEPTH */
    uint32_t edge;          /* TR_BILATERAL_BORDER or TR_BILATERAL_CLAMP */
    float depth_scale;      /* finite, >= 0; read under the DEPTH guide only, checked always */
    uint8_t border[3];      /* r, g, b of a tap outside the image under TR_BILATERAL_BORDER */
    uint8_t pad;            /* 0 */
    uint8_t spatial[225];   /* spatial[j*kw + i]: column i from the left, row j from the top; 0 beyond kw*kh */
    uint8_t pad2[3];        /* 0 */
    uint8_t range[256];     /* range[d]: the weight of a tap at distance d from the centre */
} tr_bilateral_params;
/* Filters the current frame -- what the getters mean.  Asynchronous and ordered like tr_scene_rank: frames held back are
 * submitted, a pending clear is made real, k_bilateral is enqueued on the scene's stream.  Under the COLOUR guide no depth
 * is read, so a depth left on the chip stays there; under the DEPTH guide the depth is made real first, as for
 * tr_scene_depth_of_field.  out: 3 * W * H bytes of device memory or of memory from tr_host_alloc, apart from every frame
 * buffer of the scene; every byte is written and the scene's frame stays.  out == NULL: IN PLACE, through the scene's
 * scratch frame (a tap reads neighbours) -- every later consumer sees the filtered frame, the colour fast-clear flags
 * follow (a tile is flagged only where it is zeros in every byte), z, the winner words and the shadow buffer stay;
 * calling it twice filters twice.  A tile whose existing 3 x 3 neighbourhood is flagged clean in colour, with no non-zero
 * border colour in reach (TR_BILATERAL_CLAMP, a border of 0, or a halo inside the image), is 0 under both guides: it is
 * stored without a load, of colour or of depth.  A colour texel behind a raised colour flag counts as zeros, a depth
 * behind a raised depth flag as f32::MIN; neither is loaded.  A scene that is logically cleared under TR_BILATERAL_CLAMP
 * or a border of 0: zeros out of place, nothing in place, no kernel; otherwise the clear is made real and the kernel runs.
 * TR_E_INVALID, each text opening with the call's name: a null scene or params, a wrong struct_size, an even or
 * out-of-range kw or kh, spatial weights outside the window, an all-zero window, an unknown guide or edge, a depth_scale
 * that is negative, infinite or a NaN, pad or pad2 != 0; a BAND scene (tr_options.band_row0/1 set: the taps at a band's
 * border lie in another rank's rows); ordinary host memory as `out`, a pinned buffer that is too small, an `out` that
 * overlaps a frame buffer of the scene.  The parameters are checked first, then the band, then `out`. */
int tr_scene_bilateral(tr_scene *s, const tr_bilateral_params *p, void *out /* or NULL */);
/* The same into any host memory (3 * W * H bytes): waits for the scene first, filters into a buffer of the library's,
 * copies out and returns the frame's sticky status, like tr_scene_get_ranked.  The scene's frame stays. */
int tr_scene_get_bilateral(tr_scene *s, const tr_bilateral_params *p, uint8_t *rgb);
/* The rule above on the host (no GPU needed), by the inline functions k_bilateral shares.  rgb and out: 3 * width *
 * height bytes, row 0 = top; out must not be rgb.  z: width * height floats, x + y*W, y up; NULL is allowed under the
 * COLOUR guide, which does not read it.  The same parameter checks; a width or height of 0 returns TR_OK. */
int tr_bilateral_host(uint32_t width, uint32_t height, const uint8_t *rgb /* row 0 = top */, const float *z /* x + y*W, y up */,
                      uint8_t *out /* != rgb */, const tr_bilateral_params *p);

/* YUV output: the scene's CURRENT frame, or any rgb8 image on the device, converted on the device to 8-bit YCbCr planes --
 * the form encoders and video files take, 1.5 bytes a pixel in 4:2:0 where rgb8 has 3 -- as the chain's very last step
 * (render, composite, ..., resize, TO_YUV, read back).  The source F is the image tr_scene_get_frame_buffer would return:
 * W x H, row 0 = top, rgb8; the output has its orientation and is tightly packed (no pitch).  cw = (W + 1) / 2, ch =
 * (H + 1) / 2.
 *   TR_YUV_I420  Y (W x H), U (cw x ch), V (cw x ch), in this order                        W H + 2 cw ch bytes
 *   TR_YUV_NV12  Y (W x H), then ONE plane of cw x ch interleaved (U, V) byte pairs        W H + 2 cw ch bytes
 *   TR_YUV_I444  Y, U, V, each W x H                                                       3 W H bytes
 * Coefficients, in units of 1 / 65536, rows (r, g, b): the nearest integers to the real matrix (Kr, Kb = 0.299, 0.114 for
 * TR_YUV_BT601 and 0.2126, 0.0722 for TR_YUV_BT709; TR_YUV_LIMITED scales Y by 219 / 255 and chroma by 224 / 255), the
 * green entry adjusted so that a Y row sums to the rounded scale and a chroma row to exactly 0:
 *   601 full     Y 19595 38470 7471   U -11058 -21710 32768   V 32768 -27439 -5329   y0 0
 *   601 limited  Y 16829 33039 6416   U  -9714 -19070 28784   V 28784 -24103 -4681   y0 16
 *   709 full     Y 13933 46871 4732   U  -7509 -25259 32768   V 32768 -29763 -3005   y0 0
 *   709 limited  Y 11966 40254 4064   U  -6596 -22188 28784   V 28784 -26145 -2639   y0 16
 * Per pixel, in i32 with arithmetic shifts:  Y = (yr R + yg G + yb B + (y0 << 16) + 32768) >> 16.  For TR_YUV_I444, U and
 * V have the same form with their own rows and 128 in the place of y0.  For 4:2:0, chroma sample (i, j) covers columns 2i
 * and min(2i + 1, W - 1) and rows 2j and min(2j + 1, H - 1) -- at an odd edge the last column or row counts twice --, Rs,
 * Gs, Bs are the sums of those four pixels (0..1020) and the result is rounded once:
 *     U = (ur Rs + ug Gs + ub Bs + (128 << 18) + (1 << 17)) >> 18, V alike with the V row.
 * Every result is then clamped to 0..255.  It follows: the clamp only acts at the top (full range: pure blue gives U = 256
 * and pure red V = 256 before it; limited range stays within 16..235 / 16..240; nothing goes negative); a grey v gives
 * Y = v in full range and U = V = 128 in every table; black gives (y0, 128, 128); every accumulator stays below 2^27.  The
 * 4:2:0 siting is the centred one (C420jpeg in a Y4M header).  This Y is NOT tr_frame_stats' 8-bit luma (54, 183, 19).
 * No gamma: the bytes are converted as stored. */
#define TR_YUV_I420 0u
#define TR_YUV_NV12 1u
#define TR_YUV_I444 2u
#define TR_YUV_BT601 0u
#define TR_YUV_BT709 1u
#define TR_YUV_FULL 0u
#define TR_YUV_LIMITED 1u
typedef struct tr_yuv_params {
    uint32_t layout; /* TR_YUV_I420, TR_YUV_NV12 or TR_YUV_I444 */
    uint32_t matrix; /* TR_YUV_BT601 or TR_YUV_BT709 */
    uint32_t range;  /* TR_YUV_FULL or TR_YUV_LIMITED */
    uint32_t flags;  /* 0 */
} tr_yuv_params;
/* The bytes of all planes of a width x height image (each 1..8192); 0, with a tr_last_error text, for an unknown layout
 * or such a size. */
size_t tr_yuv_bytes(uint32_t width, uint32_t height, uint32_t layout);
/* Plane `plane` (0: Y; I420 and I444: 1 U, 2 V; NV12: 1 the pairs): the offset of its first byte, its width and height in
 * samples and the bytes from one sample to the next of its kind (NV12's pairs: cw x ch, step 2; else 1).  TR_E_INVALID
 * for a null pointer, an unknown layout, a size outside 1..8192 or a plane the layout has not. */
int tr_yuv_plane(uint32_t width, uint32_t height, uint32_t layout, uint32_t plane, size_t *offset, uint32_t *w, uint32_t *h, uint32_t *step);
/* The table above as the library holds it: out10 = Y row, U row, V row, y0.  TR_E_INVALID for an unknown matrix or range. */
int tr_yuv_coefficients(uint32_t matrix, uint32_t range, int32_t *out10);
/* Converts the current frame -- what the getters mean: the last render's, a frame chosen with tr_scene_select_frame, the
 * caller's buffer after tr_scene_set_frame_buffer_device.  Asynchronous and ordered like tr_scene_resize: frames held
 * back are submitted, a pending clear is made real, k_yuv is enqueued on the scene's stream behind the renders issued so
 * far (no depth is read, so a depth left on the chip stays there), a later render is ordered behind it, the result is
 * there after tr_scene_sync.  The scene's passes issued so far count as handed on.  A 128 x 16 tile whose colour
 * fast-clear flag is up is not loaded: its Y is y0 and its chroma 128; where an odd H puts the two rows of a chroma
 * sample into two tiles, the flagged one counts as zeros and is still not read.
 * out: tr_yuv_bytes bytes of device memory at ANY address, or memory from tr_host_alloc (the kernel stores through its
 * mapped address; the buffer's sparse read-back record lapses); every byte of it is written on every call.  The planes
 * are no frame of the scene: there is no in-place form and out == NULL is refused.
 * A scene that is logically cleared (tr_scene_clear and nothing rendered since) gives the planes of black by fills
 * (hipMemsetAsync, no kernel).
 * TR_E_INVALID with a tr_last_error text that names the call, nothing changed and nothing queued: a NULL scene, params
 * or out, flags != 0, an unknown layout, matrix or range, ordinary host memory as `out`, a pinned buffer that is too
 * small, an `out` that overlaps a frame buffer of the scene, and a BAND scene (tr_options.band_row0/1 set): a chroma
 * sample's pair of rows straddles a band's border. */
int tr_scene_to_yuv(tr_scene *s, const tr_yuv_params *p, void *out);
/* The same for ANY tightly packed rgb8 image of width x height pixels (each 1..8192, row 0 = top) in device memory or in
 * memory from tr_host_alloc -- the output of tr_scene_resize, tr_scene_resolve or tr_scene_warp --, enqueued on the scene's
 * stream behind everything issued so far.  No flags are used: every pixel is read.  Also refused: an `rgb` that is
 * ordinary host memory or a pinned block that is too small, and an `rgb` that overlaps `out`.  Band scenes may call it. */
int tr_scene_to_yuv_from(tr_scene *s, const void *rgb, uint32_t width, uint32_t height, const tr_yuv_params *p, void *out);
/* The current frame's planes into any host memory (tr_yuv_bytes bytes): waits for the scene first, converts into a buffer
 * of the library's, copies out and returns the frame's sticky status, like tr_scene_get_resized. */
int tr_scene_get_yuv(tr_scene *s, const tr_yuv_params *p, uint8_t *planes);
/* The rule above on the host (no GPU needed), by the very inline functions k_yuv calls.  rgb: 3 * width * height bytes,
 * out: tr_yuv_bytes bytes, both row 0 = top; out must not be rgb.  The same parameter checks. */
int tr_yuv_host(uint32_t width, uint32_t height, const uint8_t *rgb, const tr_yuv_params *p, uint8_t *out /* != rgb */);

/* Layers: a SECOND image blended into the scene's CURRENT frame on the device -- a backdrop under the render, a
 * watermark, title or picture-in-picture over it, a vignette or grain (a mask multiplied or added), a cross-fade, the
 * difference of two frames -- by one exact rule.  The frame F is W x H, row 0 = top, as tr_scene_get_frame_buffer
 * returns it.  The layer L is width x height pixels (each 1..8192) of TR_LAYER_RGB8 (3 bytes a pixel) or TR_LAYER_RGBA8
 * (4, alpha last), row 0 = top, rows `stride` bytes apart (0: tightly packed; else at least width * bytes per pixel).
 * Its top-left pixel lands on frame pixel (x, y); x and y are signed, the layer may hang over any edge or miss the
 * frame.  For a frame pixel P inside the layer's rectangle, s is the layer's pixel there and d the frame's; per channel:
 *   coverage  a = A * opacity, A the layer's alpha byte (255 for RGB8), opacity 0..256: a is 0..65280.
 *             TR_LAYER_KEY: a layer pixel whose rgb equals key[0..2] has a = 0 (allowed with RGBA8: the rgb is compared).
 *             TR_LAYER_WHERE_DRAWN: a = 0 where the frame's own depth at P says nothing is drawn (bits(z) ==
 *             bits(f32::MIN)) -- the layer tints the model only.  TR_LAYER_WHERE_UNDRAWN: a = 0 where something is
 *             drawn -- a backdrop under the render.  The two exclude each other.
 *   blend     b = s (TR_LAYER_NORMAL), min(255, s + d) (ADD), (s d + 127) / 255 (MULTIPLY), 255 - ((255 - s)(255 - d) +
 *             127) / 255 (SCREEN), max(s, d) (LIGHTEN), min(s, d) (DARKEN), |s - d| (DIFFERENCE).
 *   output    (b a + d (65280 - a) + 32640) / 65280, rounded once.
 * A frame pixel outside the rectangle is unchanged.  It follows: opacity 0 or A = 0 leaves d; A = 255 at opacity 256
 * gives exactly b; NORMAL with an opaque layer of the frame's size at (0, 0) copies the layer; MULTIPLY by 255 and ADD of
 * 0 are identities; DIFFERENCE of a frame with itself is black.  ONLY COLOUR CHANGES: z, winner words and the shadow
 * buffer stay, so a backdrop pixel is still "not drawn" to a later tr_scene_composite, tr_scene_outline, depth of field
 * or another WHERE layer.  A pixel depends on itself and on the layer alone: the rule works in place. */
#define TR_LAYER_NORMAL 0u
#define TR_LAYER_ADD 1u
#define TR_LAYER_MULTIPLY 2u
#define TR_LAYER_SCREEN 3u
#define TR_LAYER_LIGHTEN 4u
#define TR_LAYER_DARKEN 5u
#define TR_LAYER_DIFFERENCE 6u
#define TR_LAYER_RGB8 0u
#define TR_LAYER_RGBA8 1u
#define TR_LAYER_KEY 0x1u
#define TR_LAYER_WHERE_DRAWN 0x2u
#define TR_LAYER_WHERE_UNDRAWN 0x4u
#define TR_LAYER_MAX_SIDE 8192
typedef struct tr_layer_params {
    uint32_t mode;     /* TR_LAYER_NORMAL .. TR_LAYER_DIFFERENCE */
    uint32_t format;   /* TR_LAYER_RGB8 or TR_LAYER_RGBA8 */
    uint32_t flags;    /* TR_LAYER_KEY, and at most one of TR_LAYER_WHERE_DRAWN / TR_LAYER_WHERE_UNDRAWN */
    uint32_t opacity;  /* 0..256 */
    int32_t x, y;      /* where the layer's top-left pixel lands in the frame (row 0 = top) */
    uint32_t width, height; /* the layer's size in pixels, each 1..TR_LAYER_MAX_SIDE */
    uint32_t stride;   /* bytes from one row of the layer to the next; 0: width * bytes per pixel */
    uint8_t key[4];    /* r, g, b of TR_LAYER_KEY; key[3] is not looked at */
} tr_layer_params;
/* Blends `image` into the current frame -- what the getters mean: the last render's, a frame chosen with
 * tr_scene_select_frame, the caller's buffer after tr_scene_set_frame_buffer_device.  Asynchronous and ordered like
 * tr_scene_grade: frames held back are submitted, a pending clear is made real, k_layer is enqueued on the scene's stream
 * behind the renders issued so far, a later render is ordered behind it, the result is there after tr_scene_sync; the
 * scene's passes issued so far count as handed on.  Depth is read only with a WHERE flag (then a depth left on the chip
 * is made real first, as for tr_scene_outline); without one it stays where it is.
 * image: the layer in device memory at ANY byte address, or memory from tr_host_alloc (the kernel loads through its
 * mapped address); stride * (height - 1) + width * bytes per pixel bytes of it are read and no byte outside them.
 * out == NULL: in place, by the kernel itself -- no scratch frame, no copy.  Only tiles the rectangle touches are
 * visited; a 128 x 16 tile whose colour fast-clear flag is up counts as zeros without a load and, where the result can
 * differ from zeros, is stored whole with its flag lowered (MULTIPLY and DARKEN leave it black behind its flag).  Every
 * later consumer sees the layered frame; calling it twice blends twice.  A layer that misses the frame, or opacity 0,
 * queues nothing.
 * Otherwise out: 3 W H bytes of device memory or memory from tr_host_alloc, apart from every frame buffer of the scene;
 * every byte of it is written, the blended rectangle and a copy of the rest, and the scene's frame stays as it is.  A
 * logically cleared scene gives the layer over black.
 * TR_E_INVALID with a tr_last_error text that names the call, nothing changed and nothing queued: a NULL scene, params
 * or image; an unknown mode, format or flag; both WHERE flags; opacity > 256; width or height 0 or above 8192; a
 * non-zero stride below the row's bytes; a BAND scene (tr_options.band_row0/1); `image` or `out` that is ordinary host
 * memory or a pinned block that is too small; `out` overlapping a frame buffer of the scene; `image` overlapping `out`
 * or a frame buffer of the scene. */
int tr_scene_layer(tr_scene *s, const tr_layer_params *p, const void *image, void *out /* or NULL */);
/* The same with src's CURRENT frame as the layer (rgb8, of src's size, which may differ from dst's): p->format must be
 * TR_LAYER_RGB8 and p->width, p->height and p->stride 0 -- they are taken from src.  A tile of src behind a raised colour
 * flag is taken as zeros and never loaded; a logically cleared src is a layer of zeros.  Stream ordering between the
 * two scenes as in tr_scene_composite: the launch is behind src's work issued so far, a later render of src behind the
 * launch, and both scenes' passes count as handed on.  src's frame, depth and flags are only read.  Also refused:
 * src == dst, scenes on different devices, a band scene on either side, a src wider or higher than 8192, an `out` that
 * overlaps a frame buffer of src. */
int tr_scene_layer_from_scene(tr_scene *dst, const tr_layer_params *p, tr_scene *src, void *out /* or NULL */);
/* The layered frame into any host memory (3 W H bytes): waits for the scene first, blends into a buffer of the library's,
 * copies out and returns the frame's sticky status, like tr_scene_get_graded.  The scene's frame stays as it is. */
int tr_scene_get_layered(tr_scene *s, const tr_layer_params *p, const void *image, uint8_t *rgb);
/* The rule above on the host (no GPU needed), by the very inline functions k_layer calls.  rgb and out: 3 * width * height
 * bytes, row 0 = top; out may be rgb.  z: width * height floats, index x + y * width with y UP (tr_scene_read_z_f32); NULL
 * without a WHERE flag.  image: any host memory.  The same parameter checks; width and height are the FRAME's, at least 1. */
int tr_layer_host(uint32_t width, uint32_t height, const uint8_t *rgb, const float *z /* NULL without a WHERE flag */,
                  const tr_layer_params *p, const uint8_t *image, uint8_t *out /* may be rgb */);

/* Depth ramp: the scene's CURRENT frame coloured by its own depth on the device -- fog with any falloff, a depth cue
 * (MULTIPLY), a grey or false-colour depth view, contour bands, a depth slice or matte, a glow by distance (ADD): each
 * is only another table.  One rule for every pointwise depth operation, as tr_scene_grade is for pointwise colour.
 * The table holds n entries of rgba8, n = 2..TR_RAMP_MAX_N; entry k is rgba[4 k .. 4 k + 3].  For a pixel with depth z
 * (what tr_scene_read_z_f32 returns, index x + y * width, y up) and stored colour d:
 *   position  bits(z) == bits(f32::MIN): nothing is drawn there; the pixel takes no position and the entry `undrawn`
 *             (r in bits 0..7, g in 8..15, b in 16..23, alpha in 24..31).  Otherwise p = (fl(fl(z - z0) * scale)) as u32:
 *             every f32 operation rounds once, `as u32` truncates, saturates and takes NaN and negatives to 0.  p counts
 *             1/256 of a table step.  scale may be negative: nearer is LARGER in this renderer, so a ramp that grows with
 *             distance has scale < 0.  With pmax = (n - 1) * 256: p = min(p, pmax); with TR_RAMP_REPEAT p = p % pmax.
 *             i = p >> 8, f = p & 255, j = min(i + 1, n - 1).
 *   entry     per channel c of r, g, b, a: e_c = (E_i[c] * (256 - f) + E_j[c] * f + 128) >> 8.
 *   blend     coverage cov = e_a * opacity, opacity 0..256; the output is the layer rule's (above): b from `mode`
 *             (TR_LAYER_NORMAL .. TR_LAYER_DIFFERENCE) of s = e_rgb and d, then (b cov + d (65280 - cov) + 32640) / 65280.
 * So cov == 0 leaves d; alpha 255 at opacity 256 under NORMAL gives the entry's colour exactly (a depth view); an
 * `undrawn` alpha of 0 leaves the background alone, a fog-coloured `undrawn` with alpha 255 fogs it out.  Only colour
 * changes: z, winner words and the shadow buffer stay.  A pixel depends on itself alone: the rule works in place. */
#define TR_RAMP_MAX_N 1024
#define TR_RAMP_REPEAT 0x1u
typedef struct tr_ramp_params {
    float z0;          /* the depth of position 0; finite */
    float scale;       /* positions (1/256 of a table step) per unit of depth; finite, not 0, either sign */
    uint32_t mode;     /* TR_LAYER_NORMAL .. TR_LAYER_DIFFERENCE */
    uint32_t opacity;  /* 0..256 */
    uint32_t undrawn;  /* the entry of a pixel that is not drawn: r | g << 8 | b << 16 | alpha << 24 */
    uint32_t flags;    /* TR_RAMP_REPEAT or 0 */
    uint32_t reserved[2]; /* 0 */
} tr_ramp_params;
/* Sets (copies) the scene's ramp table and returns when the copy is done; changing the table waits for the scene's queued
 * work first (frames issued so far keep the table they were issued under), like tr_scene_set_lut.  n == 0 drops the table
 * (rgba may then be NULL).  TR_E_INVALID with a tr_last_error text, nothing changed: a NULL scene, n == 1,
 * n > TR_RAMP_MAX_N, NULL rgba with n > 0. */
int tr_scene_set_ramp(tr_scene *s, uint32_t n, const uint8_t *rgba /* 4*n, host */);
/* Ramps the current frame.  Asynchronous and ordered like tr_scene_layer: frames held back are submitted, a pending clear
 * is made real, a depth left on the chip is made real (the stage always reads depth), k_ramp is enqueued on the scene's
 * stream; the result is there after tr_scene_sync, and the scene's passes issued so far count as handed on.
 * out == NULL: in place, by the kernel itself -- no scratch frame, no copy.  A 128 x 16 tile in which nothing is drawn
 * loads no depth; with an `undrawn` coverage of 0 it is not touched.  A tile whose colour fast-clear flag is up counts as
 * zeros without a load and is stored whole with its flag lowered (MULTIPLY and DARKEN leave it black behind its flag).
 * Otherwise out: 3 W H bytes of device memory at any byte address or memory from tr_host_alloc, apart from every frame
 * buffer of the scene; every byte of it is written and the scene's frame stays as it is.  A logically cleared scene is
 * `undrawn` over black everywhere: where that is black nothing runs (zeros out of place, nothing in place).
 * TR_E_INVALID with a tr_last_error text that names the call, nothing changed and nothing queued: a NULL scene or params;
 * z0 not finite; scale not finite or 0; mode > TR_LAYER_DIFFERENCE; opacity > 256; an unknown flag; reserved not 0; a
 * scene without a table; a BAND scene (tr_options.band_row0/1); `out` that is ordinary host memory, a pinned block that
 * is too small, or overlaps a frame buffer of the scene. */
int tr_scene_ramp(tr_scene *s, const tr_ramp_params *p, void *out /* or NULL */);
/* The ramped frame into any host memory (3 W H bytes): waits for the scene first, ramps into a buffer of the library's,
 * copies out and returns the frame's sticky status, like tr_scene_get_layered.  The scene's frame stays as it is. */
int tr_scene_get_ramped(tr_scene *s, const tr_ramp_params *p, uint8_t *rgb);
/* The rule above on the host (no GPU needed), by the very inline functions k_ramp calls.  rgb and out: 3 * width * height
 * bytes, row 0 = top; out may be rgb.  z: width * height floats, index x + y * width with y UP.  table: 4 * n bytes.  The
 * same parameter checks; n must be 2..TR_RAMP_MAX_N, width and height at least 1. */
int tr_ramp_host(uint32_t width, uint32_t height, const uint8_t *rgb, const float *z, const tr_ramp_params *p, uint32_t n,
                 const uint8_t *table, uint8_t *out /* may be rgb */);
/* positions[k] = p of the depth z[k] under the parameters and a table of n entries -- after the clamp or the REPEAT --,
 * 0xFFFFFFFF for a depth that is not drawn: the means to choose z0 and scale, as tr_dof_coc is for a focus. */
int tr_ramp_positions(const tr_ramp_params *p, uint32_t n, uint32_t count, const float *z, uint32_t *positions);
/* Diagnostic, as tr_scene_debug_grade_grid: k_ramp's workgroups are persistent; every later k_ramp launch of the scene
 * starts at most `cap` of them (0: no cap, the default), so that each walks more tiles.  The result does not change.
 * Returns the number of workgroups of the scene's most recent k_ramp launch (0: there has been none). */
int tr_scene_debug_ramp_grid(tr_scene *s, uint32_t cap);

/* Lines: a table of straight segments kept on the scene, drawn into the scene's CURRENT frame on the device and
 * depth-tested against the frame's own z -- a wireframe over or instead of the shaded mesh, a skeleton, a bounding box,
 * axes, a grid, normals, a camera path, a crosshair, a frame around an inset.  The first stage that draws.
 * A segment is a tr_line.  Coordinates are the renderer's own raster coordinates (the reference's vertex_t_raster, what
 * tr_project_points gives): x runs right and y runs UP; pixel (x, y) is frame row H - 1 - y and depth index x + y * W (what
 * tr_scene_read_z_f32 returns).  Endpoints may lie outside the frame; |x|, |y| <= 2^20; z finite with |z| <= 2^100.
 *   pixels  dx = x1 - x0, dy = y1 - y0; the major axis is x iff |dx| >= |dy|.  The endpoints are swapped (with their z) iff
 *           the second one's major coordinate is smaller, so a segment and its reverse cover the same pixels.  With n =
 *           |d_major| and db = d_minor after the swap, step k = 0..n is major a0 + k, minor b0 + floor((2 k db + n) / (2 n)),
 *           exactly; n == 0 is the single pixel (x0, y0).  With `width` w = 1..15 a step covers the minor offsets
 *           -((w - 1) / 2) .. +(w / 2) (butt caps).  Pixels outside the frame are dropped.
 *   depth   t = (float)k / (float)n (0 if n == 0), z = z0 + (z1 - z0) * t, zl = z + depth_bias: every f32 operation rounded
 *           once, the quotient correctly, nothing contracted.
 *   test    with TR_LINES_DEPTH_TEST a candidate survives at a pixel iff !(zl <= zbuf), the reference's own comparison: it
 *           survives a NaN depth and f32::MIN (nothing drawn).  Without the flag every candidate survives, no depth is read.
 *   winner  among a pixel's survivors the greatest key wins -- the total order of the bits of zl,
 *           bits ^ (bits >> 31 ? 0xFFFFFFFF : 0x80000000): the nearest --, ties to the greatest segment index.  With
 *           TR_LINES_PAINTER the greatest index wins whatever its depth (drawing order).
 *   output  only the winner touches the pixel: coverage a = rgba[3] * opacity (0..65280), per channel
 *           (rgb a + d (65280 - a) + 32640) / 65280, the layer rule's NORMAL.  A pixel without a winner keeps d.
 * Only colour changes: z, winner words and the shadow buffer stay.  A pixel depends on itself and the table alone: the
 * rule works in place. */
#define TR_LINES_MAX_N (1u << 20)
#define TR_LINES_MAX_WIDTH 15u
#define TR_LINES_DEPTH_TEST 0x1u
#define TR_LINES_PAINTER 0x2u
typedef struct tr_line {
    int32_t x0, y0;
    float z0;
    int32_t x1, y1;
    float z1;
    uint8_t rgba[4];
    uint32_t reserved; /* 0 */
} tr_line;
typedef struct tr_lines_params {
    uint32_t width;    /* 1..15 pixels across the minor axis */
    uint32_t opacity;  /* 0..256 */
    uint32_t flags;    /* TR_LINES_DEPTH_TEST, TR_LINES_PAINTER */
    float depth_bias;  /* added to a step's depth before the test and the order; finite.  Nearer is LARGER: > 0 lifts */
    uint32_t reserved[4]; /* 0 */
} tr_lines_params;
/* Sets (copies) the scene's table of n segments, n = 0..TR_LINES_MAX_N, and returns when the copy is done; like
 * tr_scene_set_ramp it waits for the scene's queued work first, so frames issued so far keep the table they were issued
 * under.  Every segment is validated, then the table is binned on the host into the 128 x 16 tiles of the frame: a
 * segment enters exactly the tiles in which one of its pixels at width 15 lies, computed per tile column or row from
 * the rule itself, so a diagonal across the frame lands in as many lists as it crosses tiles; no list has a capacity.
 * n == 0 drops the table (lines may then be NULL).  TR_E_INVALID with a tr_last_error text, nothing changed: a NULL
 * scene, n > TR_LINES_MAX_N, NULL lines with n > 0, a segment (named by its index) with a coordinate beyond +-2^20, a z
 * that is not finite or beyond 2^100, or reserved not 0; a table whose lists hold 2^32 entries or more. */
int tr_scene_set_lines(tr_scene *s, uint32_t n, const tr_line *lines);
/* Draws the table into the current frame.  Asynchronous and ordered like tr_scene_layer: frames held back are submitted,
 * a pending clear is made real, under TR_LINES_DEPTH_TEST a depth left on the chip is made real (without the flag it
 * stays there), k_lines is enqueued on the scene's stream; the result is there after tr_scene_sync, and the scene's
 * passes issued so far count as handed on.
 * out == NULL: in place, by the kernel itself.  Only the tiles with a list are visited; a tile whose colour fast-clear
 * flag is up counts as zeros and is stored whole with its flag lowered iff one of its pixels has a winner, otherwise it is
 * not touched.  Otherwise out: 3 W H bytes of device memory at any byte address or memory from tr_host_alloc, apart from
 * every frame buffer of the scene; every byte of it is written (the rest of the frame is copied) and the scene's frame
 * stays as it is.  A logically cleared scene whose table reaches no tile, or opacity == 0, is its own result: zeros out
 * of place, nothing in place.
 * TR_E_INVALID with a tr_last_error text that names the call, nothing changed and nothing queued: a NULL scene or params;
 * width not 1..15; opacity > 256; an unknown flag; depth_bias not finite; reserved not 0; a scene without a table; a BAND
 * scene (tr_options.band_row0/1); `out` that is ordinary host memory, a pinned block that is too small, or overlaps a
 * frame buffer of the scene. */
int tr_scene_lines(tr_scene *s, const tr_lines_params *p, void *out /* or NULL */);
/* The frame with the lines into any host memory (3 W H bytes): waits for the scene first, draws into a buffer of the
 * library's, copies out and returns the frame's sticky status, like tr_scene_get_layered.  The scene's frame stays. */
int tr_scene_get_lined(tr_scene *s, const tr_lines_params *p, uint8_t *rgb);
/* The rule above on the host (no GPU needed), by the very inline functions k_lines calls.  rgb and out: 3 * width * height
 * bytes, row 0 = top; out may be rgb.  z: width * height floats, index x + y * width with y UP; read only under
 * TR_LINES_DEPTH_TEST (may be NULL without it).  The same checks of the parameters and of every segment; width and height
 * 1..32768; n may be 0 (lines may then be NULL). */
int tr_lines_host(uint32_t width, uint32_t height, const uint8_t *rgb, const float *z /* NULL without the test */,
                  const tr_lines_params *p, uint32_t n, const tr_line *lines, uint8_t *out /* may be rgb */);
/* For the tests: the number of non-empty tiles and the number of list entries of the scene's table (0 and 0 without one). */
int tr_scene_debug_line_bins(tr_scene *s, uint32_t *n_tiles, uint64_t *n_entries);

/* Projector: an image cast onto the model in the scene's CURRENT frame from a second camera, on the device -- a slide
 * projector or spotlight with a cookie, a decal placed from a camera, a caustics or window-light pattern, and with a second
 * scene's depth as a shadow map a second, shadow-casting light for a frame of any pipeline.  Deferred: it reads the frame's
 * colour and z alone.  The image is pw x ph pixels of 3 (rgb8) or 4 (rgba8) channels, row 0 = top, rows image_stride
 * bytes apart, at any byte address.  m (column-major) maps frame raster (x, y, z, 1) -- x right, y UP, pixel (x, y) is
 * frame row H - 1 - y and depth index x + y * W, z that depth -- to projector raster (X, Y, Z, w); tr_projector_matrix
 * builds it from two cameras.  For every DRAWN pixel (bits(z) != bits(f32::MIN)), in this order; a pixel that is not
 * drawn, or that a step rejects, keeps its colour:
 *   transform  X, Y, Z, w = ((m[i] x + m[4 + i] y) + m[8 + i] z) + m[12 + i], i = 0..3: every f32 operation rounded once,
 *              nothing contracted (tr_project_points' matrix product).  Rejected unless w > 0 and w is finite.
 *   divide     r = 1.0f / w, correctly rounded, once; u = X r, v = Y r, zp = Z r.  Rejected unless 0 <= u <= pw - 1 and
 *              0 <= v <= ph - 1 (a NaN fails).
 *   position   su = (int32)(u * 256.0f), ix = su >> 8, ax = su & 255; likewise iy, ay.  Texel (ix, iy), y UP, is image row
 *              ph - 1 - iy.
 *   image      r, g, b and alpha (255 for rgb8) bilinearly over texels (ix, iy) .. (ix + 1, iy + 1) with the warp stage's
 *              weights ((256 - ax)(256 - ay), .., sum 2^16) and rounding ((sum + 2^15) >> 16).  A texel of weight 0 is never
 *              loaded, so no byte outside the image is: at ix + 1 == pw, ax is 0.
 *   light      f = 256 without TR_PROJECTOR_OCCLUDE.  With it the occluder scene's depth zo(i, j) (index i + j * pw, y UP)
 *              makes texel (i, j) LIT iff !(zp + depth_bias < zo(i, j)): a NaN on either side is lit, a texel where the
 *              occluder drew nothing (f32::MIN) is lit.  Hard: f = 256 or 0 by the nearest texel (ix + (ax >= 128),
 *              iy + (ay >= 128)).  TR_PROJECTOR_SOFT: f = (sum of the bilinear weights of the lit texels + 128) >> 8.
 *   blend      coverage a = alpha * opacity (0..65280), a' = (a f + 128) >> 8; the pixel becomes the layer rule's blend of
 *              the sample into it under `mode` with coverage a'.
 * Nearer is LARGER: depth_bias > 0 lifts the pixel towards the projector (less self-shadowing).  With m the identity,
 * pw x ph = W x H and no occluder the result is tr_scene_layer's with TR_LAYER_WHERE_DRAWN at (0, 0); scaling all of m
 * changes nothing.  Only colour changes: z, winner words and the shadow buffer stay.  A pixel depends on itself and the
 * other inputs alone: the rule works in place.  Not here: N.L falloff (a frame keeps no normals), distance attenuation
 * (bake it into the image, or follow with tr_scene_ramp), images above 8192 x 8192, clamped or tiled images outside the
 * projector's rectangle, band scenes, filters wider than 2 x 2 (tr_scene_resize the image first), several projectors in
 * one call (call it again). */
#define TR_PROJECTOR_MAX_SIDE 8192u
#define TR_PROJECTOR_OCCLUDE 0x1u
#define TR_PROJECTOR_SOFT 0x2u /* only with TR_PROJECTOR_OCCLUDE */
typedef struct tr_projector_params {
    float m[16];          /* column-major: frame raster (x, y, z, 1) -> projector raster (X, Y, Z, w); every entry finite */
    uint32_t pw, ph;      /* the image's (and the occluder's) width and height, each 1..8192 */
    uint32_t channels;    /* 3 (rgb8) or 4 (rgba8) */
    uint32_t mode;        /* TR_LAYER_NORMAL .. TR_LAYER_DIFFERENCE */
    uint32_t opacity;     /* 0..256 */
    uint32_t flags;       /* TR_PROJECTOR_OCCLUDE, TR_PROJECTOR_SOFT */
    float depth_bias;     /* added to zp before the light test; finite */
    uint32_t reserved[9]; /* 0 */
} tr_projector_params;    /* 128 bytes */
/* Casts the image onto the current frame.  Asynchronous and ordered like tr_scene_layer: frames held back are submitted, a
 * pending clear is made real, a depth left on the chip is made real (the stage always reads depth), k_projector is
 * enqueued on the scene's stream; the result is there after tr_scene_sync, and the scene's passes issued so far count as
 * handed on.  image: pw x ph pixels in device memory or memory from tr_host_alloc, image_stride >= pw * channels; keep it
 * alive and unchanged until then.  occluder_scene: NULL without TR_PROJECTOR_OCCLUDE; with it a scene of exactly pw x ph on
 * the same device -- rendered from the projector's camera (TR_OPT_STORE_DEPTH spares the depth-only repeat); it may be s
 * itself.  Its CURRENT frame's depth is made real first and is read behind its renders issued so far, and it is not
 * rendered again before the kernel has read it (the ordering of tr_scene_composite's source); a texel of it behind a
 * raised depth fast-clear flag -- and all of a logically cleared occluder -- counts as f32::MIN: the kernel looks at the
 * flag per texel and never at the stale memory behind it.
 * out == NULL: in place, by the kernel itself.  A tile with nothing drawn loads nothing and is not touched; a tile whose
 * colour fast-clear flag is up counts as zeros and is stored whole with its flag lowered iff one of its pixels is covered
 * (drawn and accepted by every step); under TR_LAYER_MULTIPLY and TR_LAYER_DARKEN it stays black behind its flag.
 * Otherwise out: 3 W H bytes of device memory at any byte address or memory from tr_host_alloc, apart from every frame
 * buffer of the scene and from the image; every byte of it is written (the rest of the frame is copied) and the scene's
 * frame stays as it is.  A logically cleared scene is its own result: zeros out of place, nothing in place, no kernel;
 * opacity == 0 in place does nothing (out of place the frame is copied).
 * TR_E_INVALID with a tr_last_error text that names the call, nothing changed and nothing queued: a NULL scene, params or
 * image; pw or ph outside 1..8192; channels not 3 or 4; image_stride below the row's bytes; mode > TR_LAYER_DIFFERENCE; an
 * unknown flag; TR_PROJECTOR_SOFT without TR_PROJECTOR_OCCLUDE; opacity > 256; a depth_bias or an entry of m that is not
 * finite; reserved not 0; TR_PROJECTOR_OCCLUDE without an occluder scene, or an occluder scene without the flag; an
 * occluder of another size or on another device; a BAND scene (tr_options.band_row0/1) on either side; an image in
 * ordinary host memory or a pinned block that is too small; `out` that is ordinary host memory, a pinned block that is
 * too small, or overlaps a frame buffer of the scene or the image. */
int tr_scene_projector(tr_scene *s, const tr_projector_params *p, const void *image, uint32_t image_stride,
                       tr_scene *occluder_scene /* or NULL */, void *out /* or NULL */);
/* The frame with the image cast on it into any host memory (3 W H bytes): waits for the scene first, works into a buffer
 * of the library's, copies out and returns the frame's sticky status, like tr_scene_get_layered.  The scene's frame stays. */
int tr_scene_get_projector(tr_scene *s, const tr_projector_params *p, const void *image, uint32_t image_stride,
                           tr_scene *occluder_scene /* or NULL */, uint8_t *rgb);
/* For the tests: the number of k_projector launches this scene has enqueued so far (a refused call and a shortcut add
 * none).  The kernel has no entry in tr_scene_profile_read's table. */
int tr_scene_debug_projector_launches(tr_scene *s);
/* The rule above on the host (no GPU needed), by the very inline functions k_projector calls.  rgb and out: 3 * width *
 * height bytes, row 0 = top; out may be rgb.  z: width * height floats, index x + y * width with y UP.  image: any host
 * memory.  occluder_z: pw * ph floats, index i + j * pw with y UP, under TR_PROJECTOR_OCCLUDE; NULL without it.  The same
 * checks of the parameters; width and height 1..32768. */
int tr_projector_host(uint32_t width, uint32_t height, const uint8_t *rgb, const float *z, const tr_projector_params *p,
                      const void *image, uint32_t image_stride, const float *occluder_z /* or NULL */, uint8_t *out /* may be rgb */);
/* (tr_projector_matrix: below, with tr_uniforms) */

/* Relight: up to eight coloured directional, point and spot lights, with a highlight, laid on the scene's CURRENT frame
 * on the device from the frame's own depth -- a second light for a frame of any pipeline, a moving lamp per frame, and
 * followed by tr_scene_projector with an occluder a shadow-casting, falling-off, coloured lamp.  Deferred: it reads the
 * frame's colour and z alone.  u (column-major) maps frame raster (x, y, z, 1) -- x right, y UP, pixel (x, y) is frame
 * row H - 1 - y and depth index x + y * W, z that depth -- to model space: the i_vpmv of the view's tr_uniforms
 * (tr_prepare_uniforms kind 2).  eye is the camera's position in model space.  Every f32 operation is rounded once in
 * the order written, nothing contracted, '/' and sqrt IEEE's.  For every DRAWN pixel (bits(z) != bits(f32::MIN)):
 *   position   c[i] = ((u[i] x + u[4 + i] y) + u[8 + i] z) + u[12 + i], i = 0..3; accepted iff w = c[3] is finite and not
 *              0; r = 1.0f / w once, P = (c0 r, c1 r, c2 r), accepted only if all three are finite.
 *   normal     horizontally the candidates are (x + 1, y) and (x - 1, y), usable iff inside the frame, drawn and with a
 *              position; both usable: the first iff |za - zc| <= |zb - zc| (the nearer in depth; the tie takes + ; a NaN
 *              takes -), one: that one, none: no normal.  dx = P(a) - P or P - P(b).  The same vertically gives dy.
 *              N = dx x dy, V = eye - P, N = -N if N.V < 0; no normal unless N.N is finite and > 0, N.V is not NaN and
 *              V.V is finite and > 0.  n = N / sqrt(N.N), v = V / sqrt(V.V), a true division per component.
 *   light      TR_LIGHT_DIRECTIONAL: L = dir (a unit vector TOWARDS the light), att = 1.  TR_LIGHT_POINT: D = pos - P,
 *              d2 = D.D (skipped unless finite and > 0), L = D / sqrt(d2), att = 1.0f / (1.0f + falloff * d2).
 *              TR_LIGHT_SPOT: a point light with c = (-L).dir (dir: the unit axis from the lamp along its beam) and
 *              att = att * min(1, max(0, (c - cos_outer) * cone_scale)), cone_scale = 1 / (cos_inner - cos_outer).
 *              diff = n.L; nothing unless diff > 0.  With specular > 0: h = normalize(L + v), s = max(0, n.h), squared
 *              shininess_log2 times (the exponent 2^k), diff = diff + specular * s.  e = (diff * att) * intensity;
 *              q = (u32)(min(e, 16) * 256.0f), 0..4096 (a NaN gives 0); per channel acc[c] += q * colour[c].
 *   sample     s[c] = min(255, (256 * ambient[c] + acc[c] + 128) >> 8).  TR_RELIGHT_SHOW_NORMALS: instead
 *              s[c] = (u8)((n[c] * 0.5f + 0.5f) * 255.0f), the lights ignored: a normal map of the picture.  Then with
 *              TR_RELIGHT_ALBEDO s = (s d + 127) / 255 per channel, d the pixel's own colour: under TR_LAYER_ADD the
 *              result is d + d * s, a coloured light on an already shaded picture; TR_LAYER_MULTIPLY alone lights an
 *              unshaded one.
 *   blend      the layer rule's blend of s into the pixel under `mode` with coverage 255 * opacity.
 * A pixel that is not drawn, has no position or no normal keeps its colour.  Only colour changes: z, winner words and
 * the shadow buffer stay.  A pixel reads its own colour and its neighbours' DEPTH only: the rule works in place.  Not
 * here: shadows (follow with tr_scene_projector and an occluder), more than 8 lights in one call (call it again with
 * TR_LAYER_ADD), area lights, band scenes. */
#define TR_RELIGHT_MAX_LIGHTS 8u
#define TR_LIGHT_DIRECTIONAL 0u
#define TR_LIGHT_POINT 1u
#define TR_LIGHT_SPOT 2u
#define TR_RELIGHT_ALBEDO 0x1u
#define TR_RELIGHT_SHOW_NORMALS 0x2u
typedef struct tr_light {
    uint32_t kind;           /* TR_LIGHT_DIRECTIONAL, TR_LIGHT_POINT, TR_LIGHT_SPOT */
    float pos[3];            /* POINT, SPOT: where the lamp stands, in model space */
    float dir[3];            /* DIRECTIONAL: the unit vector towards the light; SPOT: the unit axis along the beam */
    uint8_t colour[4];       /* r, g, b, 0 */
    float intensity;         /* >= 0 */
    float falloff;           /* >= 0: att = 1 / (1 + falloff * distance^2) */
    float cos_outer;         /* SPOT: the cosine of the cone's outer half angle */
    float cone_scale;        /* SPOT: 1 / (cos_inner - cos_outer), > 0 */
    float specular;          /* >= 0; 0: no highlight */
    uint32_t shininess_log2; /* 0..10: the highlight's exponent is 2^k */
    uint32_t reserved[2];    /* 0 */
} tr_light;                  /* 64 bytes */
typedef struct tr_relight_params {
    float u[16];          /* column-major: frame raster (x, y, z, 1) -> model space; every entry finite */
    float eye[3];         /* the camera's position in model space; finite */
    uint8_t ambient[4];   /* r, g, b, 0 */
    uint32_t mode;        /* TR_LAYER_NORMAL .. TR_LAYER_DIFFERENCE */
    uint32_t opacity;     /* 0..256 */
    uint32_t flags;       /* TR_RELIGHT_ALBEDO, TR_RELIGHT_SHOW_NORMALS */
    uint32_t reserved[9]; /* 0 */
} tr_relight_params;      /* 128 bytes */
/* Lights the current frame.  Asynchronous and ordered like tr_scene_projector: frames held back are submitted, a pending
 * clear is made real, a depth left on the chip is made real (the stage always reads depth), k_relight is enqueued on the
 * scene's stream; the result is there after tr_scene_sync, and the scene's passes issued so far count as handed on.
 * lights: n_lights entries of host memory, copied by the call (NULL only with n_lights == 0).  n_lights == 0 is no
 * shortcut: the ambient term still blends into every pixel with a normal.
 * out == NULL: in place, by the kernel itself.  A tile with nothing drawn loads nothing and is not touched; a tile whose
 * colour fast-clear flag is up counts as zeros and is stored whole with its flag lowered iff one of its pixels changes;
 * under TR_LAYER_MULTIPLY and TR_LAYER_DARKEN it stays black behind its flag.  Otherwise out: 3 W H bytes of device
 * memory at any byte address or memory from tr_host_alloc, apart from every frame buffer of the scene; every byte of it
 * is written and the scene's frame stays as it is.  A logically cleared scene is its own result: zeros out of place,
 * nothing in place, no kernel.  opacity == 0: nothing in place, a copy of the frame out of place, and no k_relight.
 * TR_E_INVALID with a tr_last_error text that names the call, nothing changed and nothing queued: a NULL scene or params,
 * NULL lights with n_lights > 0; n_lights > 8; a kind above TR_LIGHT_SPOT; mode > TR_LAYER_DIFFERENCE; an unknown flag;
 * opacity > 256; an entry of u, of eye or a float of a light that is not finite; falloff, intensity or specular below 0;
 * a SPOT's cone_scale <= 0; shininess_log2 > 10; a fourth colour byte or a reserved word that is not 0; a BAND scene
 * (tr_options.band_row0/1); `out` that is ordinary host memory, a pinned block that is too small, or overlaps a frame
 * buffer of the scene. */
int tr_scene_relight(tr_scene *s, const tr_relight_params *p, const tr_light *lights, uint32_t n_lights, void *out /* or NULL */);
/* The lit frame into any host memory (3 W H bytes): waits for the scene first, works into a buffer of the library's,
 * copies out and returns the frame's sticky status, like tr_scene_get_projector.  The scene's frame stays. */
int tr_scene_get_relit(tr_scene *s, const tr_relight_params *p, const tr_light *lights, uint32_t n_lights, uint8_t *rgb);
/* For the tests: the number of k_relight launches this scene has enqueued so far (a refused call and a shortcut add
 * none).  The kernel has no entry in tr_scene_profile_read's table. */
int tr_scene_debug_relight_launches(tr_scene *s);
/* The rule above on the host (no GPU needed), by the very inline functions k_relight calls.  rgb and out: 3 * width *
 * height bytes, row 0 = top; out may be rgb.  z: width * height floats, index x + y * width with y UP.  The same checks
 * of the parameters; width and height 1..32768. */
int tr_relight_host(uint32_t width, uint32_t height, const uint8_t *rgb, const float *z, const tr_relight_params *p, const tr_light *lights,
                    uint32_t n_lights, uint8_t *out /* may be rgb */);
/* Step normal alone, on the host, for choosing parameters and for the tests: normals, 3 floats a pixel, and valid, a byte
 * a pixel (1: the pixel has a normal; 0: it has none and its floats are 0), both at index x + y * width with y UP like z.
 * Of p only u and eye are used, but all of it is checked. */
int tr_relight_normals_host(uint32_t width, uint32_t height, const float *z, const tr_relight_params *p, float *normals, uint8_t *valid);

/* Distance field: for every pixel of the scene's CURRENT frame the squared Euclidean distance, in pixels, to the nearest
 * SEED of that frame, on the device -- the answer to "how far is this pixel from the model?", and with it an outer glow, a
 * stroke of any width, contour rings, a soft drop shadow, an inner glow, a dilate or an erode by a disc of radius up to
 * 255: its cost does not grow with the square of the reach.  An exact integer quantity: whatever the device does, it
 * equals tr_distance_host in every bit.
 *   seeds   a pixel is a seed by `seed`: TR_DIST_SEED_DRAWN: bits(z) != bits(f32::MIN), the depth ramp's "drawn";
 *           TR_DIST_SEED_KEY: max(r, g, b) >= threshold on the stored bytes, threshold 0..255, no depth is read.
 *           TR_DIST_INVERT takes the complement: the result is then the distance inside a shape to its border.  Pixels
 *           outside the frame are never seeds.
 *   field   with R = radius, 1..TR_DIST_MAX_RADIUS: d2(x, y) = min over seeds (sx, sy) of (x - sx)^2 + (y - sy)^2 as a
 *           uint16_t where that is <= R * R, else TR_DIST_FAR; a seed has d2 == 0; R * R <= 65025 < 0xFFFF.  A frame
 *           without seeds is FAR everywhere.  Index x + r * width with row r = 0 the TOP row, like the frame buffer.
 *   ramp    the field coloured through the scene's ramp table (tr_scene_set_ramp, n entries): dq = floor(sqrt(d2 * 65536)),
 *           an exact integer square root (dq <= 65280); p = (dq * step) >> 8 in u32, step = 1..65536 table positions
 *           (1/256 of an entry) per pixel of distance: 256 is one entry a pixel.  Then exactly tr_scene_ramp's rule (above):
 *           p = min(p, pmax) or, with TR_DIST_REPEAT, p % pmax; entries i, j interpolated; coverage e_a * opacity; the
 *           layer rule's seven modes; (b cov + d (65280 - cov) + 32640) / 65280.  A FAR pixel takes the entry `far`, packed
 *           like tr_ramp_params.undrawn.  With TR_DIST_KEEP_SEEDS a seed keeps its colour: a glow or stroke around the
 *           model without touching it.  Only colour changes: z, winner words and the shadow buffer stay. */
#define TR_DIST_SEED_DRAWN 0u
#define TR_DIST_SEED_KEY 1u
#define TR_DIST_INVERT 0x1u     /* tr_distance_params.flags */
#define TR_DIST_REPEAT 0x1u     /* tr_distance_ramp_params.flags */
#define TR_DIST_KEEP_SEEDS 0x2u /* tr_distance_ramp_params.flags */
#define TR_DIST_MAX_RADIUS 255u
#define TR_DIST_FAR 0xFFFFu
typedef struct tr_distance_params {
    uint32_t seed;        /* TR_DIST_SEED_DRAWN or TR_DIST_SEED_KEY */
    uint32_t threshold;   /* 0..255; looked at under TR_DIST_SEED_KEY only, but checked always */
    uint32_t radius;      /* 1..TR_DIST_MAX_RADIUS */
    uint32_t flags;       /* TR_DIST_INVERT or 0 */
    uint32_t reserved[4]; /* 0 */
} tr_distance_params;
typedef struct tr_distance_ramp_params {
    tr_distance_params field;
    uint32_t step;        /* 1..65536: table positions (1/256 of an entry) per pixel of distance */
    uint32_t mode;        /* TR_LAYER_NORMAL .. TR_LAYER_DIFFERENCE */
    uint32_t opacity;     /* 0..256 */
    uint32_t far;         /* the entry of a FAR pixel: r | g << 8 | b << 16 | alpha << 24 */
    uint32_t flags;       /* TR_DIST_REPEAT | TR_DIST_KEEP_SEEDS */
    uint32_t reserved[3]; /* 0 */
} tr_distance_ramp_params;
/* The field of the current frame into `out`: 2 W H bytes of device memory at any 2-byte-aligned address, or memory from
 * tr_host_alloc, apart from every frame buffer of the scene; every uint16_t of it is written, the frame stays as it is.
 * Asynchronous and ordered like tr_scene_ramp: frames held back are submitted, a pending clear is made real; under
 * TR_DIST_SEED_DRAWN a depth left on the chip is made real, under TR_DIST_SEED_KEY it stays where it is.  Three kernels
 * on the scene's stream (k_dist_mask, k_dist_row, k_dist) through scratch memory kept on the scene from the first call
 * (a bit, a byte and 1/64 byte a pixel); the result is there after tr_scene_sync, and the scene's passes issued so far
 * count as handed on.  TR_E_INVALID with a tr_last_error text that names the call, nothing changed and nothing queued:
 * a NULL scene, params or out; seed > 1; threshold > 255; radius not 1..255; an unknown flag; reserved not 0; a BAND
 * scene (tr_options.band_row0/1); `out` that is ordinary host memory, a pinned block that is too small, an odd address,
 * or overlaps a frame buffer of the scene. */
int tr_scene_distance(tr_scene *s, const tr_distance_params *p, void *out);
/* The field into any host memory (W * H uint16_t): waits for the scene first, computes into a buffer of the library's,
 * copies out and returns the frame's sticky status, like tr_scene_get_ramped. */
int tr_scene_get_distance(tr_scene *s, const tr_distance_params *p, uint16_t *host);
/* Ramps the current frame by its distance field.  Ordering, `out` (3 W H bytes at any byte address, or NULL) and the
 * in-place form as tr_scene_ramp; the field goes to scratch memory of the scene (2 more bytes a pixel) and is complete
 * before the pointwise kernel (k_dist_apply) starts, so TR_DIST_SEED_KEY seeds are read before any colour changes.  In
 * place a 128 x 16 tile whose pixels are all FAR under a `far` coverage of 0 is not touched; a tile whose colour
 * fast-clear flag is up counts as zeros and is stored whole with its flag lowered (MULTIPLY and DARKEN leave it black
 * behind its flag).  The refusals of tr_scene_distance (`out` may be NULL and need not be even), and: step not 1..65536;
 * mode > TR_LAYER_DIFFERENCE; opacity > 256; a scene without a ramp table. */
int tr_scene_distance_ramp(tr_scene *s, const tr_distance_ramp_params *p, void *out /* or NULL */);
/* The frame ramped by its distance field into any host memory (3 W H bytes), like tr_scene_get_ramped. */
int tr_scene_get_distance_ramped(tr_scene *s, const tr_distance_ramp_params *p, uint8_t *rgb);
/* The rules above on the host (no GPU needed), by the very inline functions the kernels call.  rgb: 3 * width * height
 * bytes, row 0 = top; z: width * height floats, index x + y * width with y UP, may be NULL under TR_DIST_SEED_KEY;
 * out_u16: width * height uint16_t, row 0 = top; table: 4 * n bytes, n = 2..TR_RAMP_MAX_N; out: 3 * width * height
 * bytes, may be rgb.  The same parameter checks; width and height 1..32768. */
int tr_distance_host(uint32_t width, uint32_t height, const uint8_t *rgb, const float *z, const tr_distance_params *p, uint16_t *out_u16);
int tr_distance_ramp_host(uint32_t width, uint32_t height, const uint8_t *rgb, const float *z, const tr_distance_ramp_params *p, uint32_t n,
                          const uint8_t *table, uint8_t *out /* may be rgb */);
/* dq[k] = floor(sqrt(d2[k] * 65536)) and positions[k] = (dq[k] * step) >> 8 -- before the clamp or the REPEAT -- of count
 * field values d2[k] <= 65025 (TR_E_INVALID otherwise, and for a step not 1..65536); either output may be NULL. */
int tr_distance_positions(uint32_t step, uint32_t count, const uint16_t *d2, uint32_t *dq, uint32_t *positions);

/* Frame statistics: the scene's CURRENT frame reduced on the device to one record of 6192 bytes -- what a caller needs to
 * choose tr_dof_params.focus (a z value), tr_bloom_params.threshold (a brightness) or a level table for tr_scene_set_lut
 * without reading the frame back.  F is the frame as tr_scene_get_frame_buffer returns it (row 0 = top), z the depth as
 * tr_scene_read_z_f32 returns it.  A pixel TAKES PART when it lies in the window, the scene's band and the frame; the
 * window is x0, y0, w, h in output-image coordinates, w == 0 && h == 0 the whole frame, otherwise w, h >= 1 and wholly
 * inside the frame.
 *   colour (always), per pixel that takes part, over its stored u8 channels (R, G, B):
 *       hist[0][R]++   hist[1][G]++   hist[2][B]++
 *       hist[3][Y]++ with Y = (54 R + 183 G + 19 B + 128) >> 8      (integer BT.709: the weights sum to 256, Y <= 255)
 *       hist[4][max(R, G, B)]++                                      (the key tr_scene_bloom thresholds)
 *       n_pixels++
 *   depth (TR_STATS_DEPTH), per pixel that takes part and is DRAWN -- bits(z) != bits(f32::MIN), as tr_scene_composite
 *   has it:
 *       n_drawn++, and the box of drawn pixels grows: box_x0, box_y0 inclusive, box_x1, box_y1 exclusive, output-image
 *       coordinates; all four 0 when nothing is drawn
 *       a NaN z counts in n_nan and nowhere else
 *       any other z enters z_min / z_max under the total order of the key k = bits ^ (bits >> 31 ? 0xFFFFFFFF : 0x80000000)
 *       (-0.0 < +0.0), and zhist[min(255, ((z - z_lo) * z_scale) as u32)]++ -- f32, each operation rounded once, `as u32`
 *       the truncating, saturating cast of tr_dof_coc (negatives and -inf: bin 0; +inf: bin 255)
 *       where no drawn pixel that is not NaN exists, z_min and z_max hold f32::MIN
 *   Without the flag every depth field is zero and no depth is touched.
 * Everything is a count or an order statistic, so the record does not depend on the order of visits: the device equals
 * tr_frame_stats_host in every byte.  Every histogram sums to n_pixels, zhist to n_drawn - n_nan. */
#define TR_STATS_DEPTH 0x1u
typedef struct tr_stats_params {   /* 32 bytes */
    uint32_t struct_size, flags;
    uint32_t x0, y0, w, h;         /* window; w == h == 0: the whole frame */
    float z_lo, z_scale;           /* depth histogram; read only with TR_STATS_DEPTH: z_lo finite, z_scale finite and > 0 */
} tr_stats_params;
typedef struct tr_frame_stats {    /* 6192 bytes */
    uint32_t hist[5][256];         /* r, g, b, luma, max channel */
    uint32_t zhist[256];
    uint32_t n_pixels, n_drawn, n_nan;
    float z_min, z_max;
    uint32_t box_x0, box_y0, box_x1, box_y1;
    uint32_t reserved[3];          /* zeros */
} tr_frame_stats;
/* The record of the current frame -- what the getters mean: the last render's, a frame chosen with
 * tr_scene_select_frame, the caller's buffer after tr_scene_set_frame_buffer_device, a merged, shaded, averaged, blurred,
 * bloomed or graded frame -- into `out`: sizeof(tr_frame_stats) bytes of device memory, or of memory from tr_host_alloc
 * (the kernel stores through its mapped address).  Asynchronous and ordered like tr_scene_resolve: frames held back are
 * submitted, k_stats and k_stats_finish are enqueued on the scene's stream behind everything issued so far, a later render
 * is ordered behind them, the result is there after tr_scene_sync.  The scene's frame, z, flags and winner words are
 * never written.  The scene's passes issued so far count as handed on, as after tr_scene_resolve.
 * Tiles (128 x 16) whose colour fast-clear flag is up are not read: their pixels count in bin 0.  Tiles whose depth
 * fast-clear flag is up hold no drawn pixel and are not read either.
 * Without TR_STATS_DEPTH no depth is read: a depth left on the chip (see TR_OPT_STORE_DEPTH) stays there, no depth-only
 * repeat runs and no z buffer is allocated.  With it the depth is made real first, as by tr_scene_depth_of_field.
 * A BAND scene (tr_options.band_row0/1) is served: only its band's rows take part, and tr_frame_stats_merge over the
 * ranks' records gives the whole frame's.  A scene that is logically cleared (tr_scene_clear and nothing rendered since)
 * gives the record of a black frame in which nothing is drawn, and its pending clear stays pending.
 * TR_E_INVALID with a tr_last_error text, nothing queued: a NULL scene, NULL params or a NULL `out`, a wrong struct_size,
 * unknown flags, a window with exactly one of w, h zero or one that reaches outside the frame, with TR_STATS_DEPTH a z_lo
 * that is not finite or a z_scale that is not finite and positive, ordinary host memory as `out`, a pinned buffer that is
 * too small. */
int tr_scene_frame_stats(tr_scene *s, const tr_stats_params *p, void *out);
/* The same into any host memory: waits for the scene first (an overflowed frame is rendered again before it is read),
 * runs into a buffer of the library's, copies out and returns the frame's sticky status, like tr_scene_get_resolved. */
int tr_scene_get_frame_stats(tr_scene *s, const tr_stats_params *p, tr_frame_stats *host);
/* The rule above on the host (no GPU needed), by the very inline functions the kernels call.  rgb: 3 * width * height
 * bytes, row 0 = top; z: width * height floats, index x + y * width with y up (tr_scene_read_z_f32), read only with
 * TR_STATS_DEPTH and may be NULL without it.  The same checks of the parameters against width and height. */
int tr_frame_stats_host(uint32_t width, uint32_t height, const uint8_t *rgb, const float *z /* or NULL without the flag */,
                        const tr_stats_params *p, tr_frame_stats *out);
/* The record of the union of two DISJOINT pixel sets from their two records, into dst: counts add, z_min / z_max merge
 * under the key's order (a side without a drawn non-NaN pixel does not take part), the boxes unite (a side with nothing
 * drawn does not take part).  Both records come from calls with the same z_lo and z_scale.  Host only. */
int tr_frame_stats_merge(tr_frame_stats *dst, const tr_frame_stats *src);   /* host: the record of the union of two disjoint pixel sets */
/* Diagnostic, as tr_scene_debug_grade_grid: k_stats' workgroups are persistent -- at most one a compute unit and never
 * more than there are tiles.  `cap` is stored on the scene: every later k_stats launch of that scene starts
 * min(cap, that number) workgroups, each of which then walks more tiles, and k_stats_finish sums that many partial
 * records; not a byte of the result changes.  cap == 0: no cap, the default.  Returns the number of workgroups of the
 * scene's most recent k_stats launch (0: there has been none), or TR_E_INVALID for a NULL scene. */
int tr_scene_debug_stats_grid(tr_scene *s, uint32_t cap);                   /* as tr_scene_debug_grade_grid */

/* Dynamic textures (nothing of the kind upstream, whose four images are moved into Scene::new and never change): one of a
 * scene's images -- `which` = 0..3 in tr_scene_create's order: texture, normal_map, normal_map_tangent, specular_map --
 * replaced on the device, from host memory, from device memory or from another scene's (or the scene's own) current
 * frame: an animated or painted texture without a new scene, and render-to-texture without a read-back -- a screen inside
 * a scene, an impostor, a picture of model A on model B, feedback of a scene's own last frame.
 * The rule: the image is w x h tightly packed rgb8, row 0 = top -- image::RgbImage, and exactly what
 * tr_scene_get_frame_buffer returns.  After the call texture `which` of the scene IS that image: every render issued
 * later, in every pipeline and on every path (per-frame, held back and fused, tr_scene_render_frames*, the split
 * shadow / colour passes), draws bit for bit what a scene created with tex[which] replaced by that image draws -- colour,
 * z, winner words, shadow buffer and device status (TR_E_OOB_LOOKUP included).  w and h must equal the replaced image's
 * own size (a texture is not resized: TR_E_INVALID), so whether the scene keeps a texel set, the set's layout and the
 * choice of the lit path never change.
 * Ordering: the three setters are asynchronous.  Frames tr_scene_render holds back on the scene are submitted first and
 * keep the old texture, as do all frames issued earlier, a frame whose read-back is still queued included; k_pack_texels
 * is enqueued on the scene's stream behind all of them.  The scene's passes issued so far count as handed on, as after
 * tr_scene_composite: a bin overflow among them is reported (TR_E_BIN_OVERFLOW), never repaired by a re-render, which
 * would draw the new texture.  Kept frames (tr_scene_select_frame) stay what they are.
 * tr_scene_set_texture: host memory, copied before the call returns (through a device staging buffer on a stream of
 * the library's: the copy does not queue behind the scene's renders; with more than eight such calls in flight the
 * oldest is waited for).
 * tr_scene_set_texture_device: rgb_device is 3 * w * h bytes of device memory, or memory from tr_host_alloc.  producer:
 * the scene whose stream produced it (tr_scene_resolve, tr_scene_accumulate, tr_scene_depth_of_field with `out`): the
 * kernel runs behind producer's work -- an event on its stream -- and producer's stream then waits for the kernel, the way
 * tr_scene_composite orders dst behind src.  producer == NULL: the caller guarantees that rgb_device is complete with
 * respect to the scene's stream, and keeps it unchanged until the kernel has run (tr_scene_sync).
 * tr_scene_set_texture_from_frame: src's CURRENT frame as the getters mean it -- the last render's, a kept frame chosen
 * with tr_scene_select_frame, a caller's buffer, a merged, shaded, averaged or blurred frame -- becomes dst's image;
 * src's frame size must equal the texture's size; src == dst is allowed (feedback).  What src holds back is submitted
 * first.  A logically cleared src (tr_scene_clear and nothing rendered since) gives an image of zeros.  Tiles (128 x 16)
 * whose colour-clean flag is up in src are not read: their texels are zeros.  Ordered behind src like a producer.
 * TR_E_INVALID with a tr_last_error text, nothing changed and nothing queued: a NULL scene, image or pointer, which > 3,
 * a size that is not the replaced image's, ordinary host memory as rgb_device, a producer or src on another device, a
 * band scene (tr_options.band_row0/1) as src, rgb_device overlapping the scene's own texel arrays.
 * tr_scene_read_texture: image `which` as the scene holds it now, 3 * w * h bytes; synchronizes. */
int tr_scene_set_texture(tr_scene *s, uint32_t which, const tr_image_rgb8 *image);
int tr_scene_set_texture_device(tr_scene *s, uint32_t which, const void *rgb_device, uint32_t w, uint32_t h,
                                tr_scene *producer /* or NULL */);
int tr_scene_set_texture_from_frame(tr_scene *dst, uint32_t which, tr_scene *src);
int tr_scene_read_texture(tr_scene *s, uint32_t which, uint8_t *rgb /* 3*w*h */);
/* Diagnostic: the scene's texel set (csrc/tr_texels.h: the images its colour closure reads, interleaved texel by texel
 * and tiled into 128-byte blocks; a scene whose four images differ in size has none) copied to `words`; synchronizes.
 * Returns the number of words, 0 when the scene has no set; cap_words smaller than the set: TR_E_INVALID. */
int tr_scene_debug_texel_set(tr_scene *s, uint32_t *words, size_t cap_words);
/* The set tr_scene_create builds for `pipeline_name` from four images of one size, on the host (no GPU needed), by the
 * very function tr_scene_create calls; blocks_per_row (may be NULL) receives the blocks per row of blocks.  Returns the
 * number of words; cap_words too small, images of different sizes: TR_E_INVALID. */
int tr_texel_set_host(const char *pipeline_name, const tr_image_rgb8 tex[4], uint32_t *words, size_t cap_words,
                      uint32_t *blocks_per_row);

/* Device-resident access for callers that keep the frame on the GPU. */
int tr_scene_sync(tr_scene *s);                 /* wait for queued work; returns frame status */
int tr_scene_flush(tr_scene *s);                /* hand every render issued so far to the device (the library
                                                   may hold a few back to batch them); does not wait */
void *tr_scene_frame_buffer_device(tr_scene *s); /* 3*W*H bytes, row 0 = top */
int tr_scene_set_stream(tr_scene *s, void *hip_stream);
/* Swap the render target: renders issued after the call write `frame_buffer_device` (3*W*H bytes of
 * device memory, row 0 = top; NULL = the library's own buffer); renders already issued keep theirs.
 * A pending `clear` carries over (the next render produces every pixel of the new buffer);
 * without one the new buffer's content is taken as the frame so far.  For callers that double-buffer
 * the frame, e.g. to exchange frame f between GPUs while frame f+1 renders. */
int tr_scene_set_frame_buffer_device(tr_scene *s, void *frame_buffer_device);

/* Screen-band partition of a frame over the GPUs of a node (the reference's own clamp rectangle,
 * scene.rs:236-239, cut into row bands): rank r of n renders output rows [row0, row1), row 0 = top
 * -- the values for tr_options.band_row0/1.  Bands are disjoint, ordered by rank and cover the
 * frame; they are equal (what an in-place all-gather needs) exactly when n divides height. */
int tr_band_rows(uint32_t height, uint32_t n_ranks, uint32_t rank, uint32_t *row0, uint32_t *row1);

/* Multi-GPU frame exchange without RCCL (SURVEY.md 8e's hand-tuned alternative; nothing of the kind
 * upstream).  One process per GPU.  Each rank creates its end -- 1 to 64 full-size frame buffers
 * ("slots": pass their device pointers to tr_scene_create / tr_scene_set_frame_buffer_device) -- and
 * publishes a TR_EXCHANGE_HANDLE_BYTES record; once every rank has connected to all records (in rank
 * order; the host's own rendezvous carries them), tr_exchange_all_gather(slot, offset, bytes, stream)
 * pushes bytes [offset, offset + bytes) of the local slot into the same range of every peer's slot
 * with concurrent DMA-engine copies over xGMI, after the work queued on `stream` so far, and makes
 * `stream` wait until every peer's range has arrived in the local slot.  Collective: every rank calls it
 * for the same slots in the same order.  Failures of a peer surface as TR_E_EXCHANGE from
 * tr_exchange_status / tr_exchange_read after a device-side timeout (ten seconds; the environment
 * variable TR_EXCHANGE_TIMEOUT_MS, read at create, overrides it), never as a hang. */
#define TR_EXCHANGE_HANDLE_BYTES 256
typedef struct tr_exchange tr_exchange;
int tr_exchange_create(int device, uint32_t n_ranks, uint32_t rank, uint32_t n_slots, size_t frame_bytes, tr_exchange **out);
/* The same exchange with a choice of transport.  TR_EXCHANGE_PEER: the copies described above (tr_exchange_create).
 * TR_EXCHANGE_RCCL (north_star: "RCCL all-gather of the final framebuffer over xGMI"): connect builds
 * an RCCL communicator owned by the exchange (rank 0's record carries the ncclUniqueId: the host's rendezvous only
 * moves the 256-byte records, as for the peer transport; every rank must be inside tr_exchange_connect at the same
 * time) and tr_exchange_all_gather is ONE in-place ncclAllGather on `hip_stream`; the ranks' byte ranges must then be
 * equal pieces of one range, in rank order -- tr_band_rows with a height the ranks divide.  librccl is loaded when
 * such an exchange is created; failures are TR_E_RCCL.  A Rust (or C) host needs no torch for either. */
#define TR_EXCHANGE_PEER 0
#define TR_EXCHANGE_RCCL 1
int tr_exchange_create_backend(int device, uint32_t n_ranks, uint32_t rank, uint32_t n_slots, size_t frame_bytes, int backend,
                               tr_exchange **out);
uint64_t tr_exchange_bytes_sent(tr_exchange *x); /* bytes this rank has pushed to its peers since the exchange was created */
void *tr_exchange_frame(tr_exchange *x, uint32_t slot);
int tr_exchange_export(tr_exchange *x, void *record /* TR_EXCHANGE_HANDLE_BYTES */);
int tr_exchange_connect(tr_exchange *x, const void *records /* n_ranks * TR_EXCHANGE_HANDLE_BYTES */);
int tr_exchange_all_gather(tr_exchange *x, uint32_t slot, size_t offset, size_t bytes, void *hip_stream);
/* Declares every rank's byte range of a frame (n_ranks offsets and sizes, disjoint: the bands of tr_band_rows), the same
 * on all ranks, before the first tr_exchange_all_gather.  The peer transport's dense exchange then PULLS: a rank copies
 * its peers' ranges out of their mapped slots into its own slot, and nothing but 4-byte flags is ever written into
 * another rank's memory -- a peer that is late or gone costs this rank its own frame (TR_E_EXCHANGE), never a slot the
 * owner had not opened (the push form's copy engines cannot be predicated on the error word).  tr_exchange_all_gather
 * must then be called with this rank's declared range.  NULL, NULL: back to the push form.  RCCL transport: checked, unused. */
int tr_exchange_set_ranges(tr_exchange *x, const size_t *offsets, const size_t *bytes);
/* The SPARSE form of the exchange: the band of `slot`'s frame that scene `s` renders goes to the peers tile by tile
 * (128 x 16 pixels), and a tile that holds the cleared colour here AND held it the last time this rank wrote the
 * peer's copy does not travel at all -- three quarters of a 4096x4096 frame of the reference's model.  The scene
 * knows which tiles those are (the fast-clear flags of its frame buffers: tr_scene_band_tiles); the exchange keeps
 * the record of what each peer's copy holds.  The slot must be the frame buffer the scene rendered into
 * (tr_scene_set_frame_buffer_device / tr_scene_render_frames) and nobody else may write this rank's band of the
 * peers' copies.  Same ordering and collective rules as tr_exchange_all_gather; a tr_exchange_all_gather on the slot
 * in between is allowed (it resets the record).  TR_EXCHANGE_PEER: one kernel per peer storing through the mapped
 * slots over xGMI.  TR_EXCHANGE_RCCL (a collective's sizes are fixed by the host before the frame's coverage is
 * known) and frames whose width is not a multiple of 16: the dense exchange of the band's rows.
 * tr_exchange_bytes_sent counts what really travelled (it waits for the device). */
typedef struct tr_band_tiles {
    const void *frame_buffer_device; /* the frame buffer the flags describe */
    const uint32_t *clean_device;    /* tiles_x * tiles_y flags on the device, row-major: != 0 = the tile's pixels are zeros */
    uint32_t width, height;          /* the frame */
    uint32_t tiles_x, tiles_y;       /* tile grid of the band; tiles are 128 x 16 pixels */
    int32_t first_tile_row;          /* tile row (y up, rows of 16 pixels from the bottom) of grid row 0 */
    int32_t band_y0, band_y1;        /* scene rows [y0, y1), y up, that the scene renders; buffer row = height - 1 - y */
} tr_band_tiles;
/* Queues what is still held back of the scene's frames and describes the tiles of `frame_buffer_device` (one of the
 * buffers the scene has rendered into; NULL = the current one).  The flags are read by work queued AFTER the frame
 * on the scene's stream or on a stream that waits for it. */
int tr_scene_band_tiles(tr_scene *s, const void *frame_buffer_device, tr_band_tiles *out);
int tr_exchange_all_gather_tiles(tr_exchange *x, uint32_t slot, const tr_band_tiles *tiles, void *hip_stream);
int tr_exchange_status(tr_exchange *x);
int tr_exchange_read(tr_exchange *x, uint32_t slot, void *host, size_t bytes); /* waits for the device, copies a slot out */
/* Tearing a peer exchange down takes two steps when its ranks go on living (they create another exchange, say): a rank
 * must not FREE slots a peer still has mapped (what HIP leaves undefined for exported memory), so every rank first
 * unmaps its peers' slots and flags -- tr_exchange_disconnect: waits for the device, after which the exchange can only
 * be destroyed --, the host's rendezvous confirms that all have (a barrier), and then each destroys its end.
 * tr_exchange_destroy alone does both at once: fine when the process ends anyway. */
int tr_exchange_disconnect(tr_exchange *x);
void tr_exchange_destroy(tr_exchange *x);

/* Diagnostic (TR_OPT_TILE_STAMPS): for each tile of the last colour pass {start, end} in 100 MHz
 * ticks, polygons in its bin, hardware id, {bin staged, coverage done} ticks, 2 spare.  `out`
 * holds 8 * n_tiles entries; returns n_tiles. */
int tr_scene_debug_tile_stamps(tr_scene *s, uint64_t *out, uint32_t cap_tiles);

/* Per-kernel device timing with HIP events on the scene's stream (bench roofline leg). */
typedef struct tr_kernel_time {
    char name[32];
    uint64_t launches;
    double total_ms;
    uint64_t frames; /* frames those launches covered (= launches, except for tr_scene_render_frames' fused launches) */
} tr_kernel_time;
int tr_scene_profile_enable(tr_scene *s, int on);
/* Fills up to `cap` entries, returns the number of kernels or a negative status. */
int tr_scene_profile_read(tr_scene *s, tr_kernel_time *out, int cap);
/* Frame times of the profiled renders: microseconds between the completions of consecutive frames'
 * (colour-pass) tile kernels, in issue order.  Returns how many were written (<= cap). */
int tr_scene_profile_frame_intervals(tr_scene *s, float *out_us, int cap);

/* Device self-test of the arithmetic primitives the kernels substitute for the reference's:
 * Rust `as` casts (f32 -> u32 / i32 / u8) and x / d through a shared reciprocal.  Inputs and
 * outputs are host arrays of n elements; div_ref receives the device's plain x / d. */
int tr_selftest_device_math(int device, const float *x, const float *d, uint32_t n, uint32_t *out_u32,
                            int32_t *out_i32, uint32_t *out_u8, float *out_div, float *out_div_ref);

/* Device self-test of the shadow-buffer lookup of the shadow / occlusion closures (shader.rs:774-778, 909-912,
 * 932-935: (round(x) as u32 + round(y) as u32 * width) as usize, wrapping) as the kernels perform it THROUGH the
 * shadow buffer's per-tile fast-clear flags: `stale` is a width x height buffer whose tiles with a non-zero flag in
 * `sclean` (one word per 128 x 16 tile, row-major) hold arbitrary values, `plain` the same buffer with those tiles
 * written as f32::MIN.  For each of the n coordinates the value bits and error bits (4 = index out of range) of the
 * plain lookup in `plain` and of the flagged lookup in `stale` are returned; they must be equal -- also for a
 * column beyond the row and for a row k * 2^32 / width + r, which wraps around 2^32 back into the buffer. */
int tr_selftest_shadow_fetch(int device, uint32_t width, uint32_t height, const float *plain, const float *stale,
                             const uint32_t *sclean, uint32_t n, const float *x, const float *y, uint32_t *out_plain,
                             uint32_t *out_flagged, uint32_t *err_plain, uint32_t *err_flagged);

/* Exhaustive device check of the kernels' own correctly rounded reciprocal (which = 0) and square
 * root (which = 1) for pixel pairs (csrc/tr_pk.h rcp2 / sqrt2: hardware estimate + fused residual
 * corrections) against the compiler's IEEE `1.0f / x` and `sqrtf`: every f32 with binary exponent in
 * [exp_lo, exp_hi].  which = 2: the colour channels' cast-and-insert (v_cvt_pk_u8_f32) against the Rust `as u8` it
 * stands for, x and -x; exp_lo = -127 .. exp_hi = 128 covers every f32 (zeros, subnormals, infinities, NaNs).
 * n_bad counts differing results, bad_bits receives up to 16 of the arguments. */
int tr_selftest_device_unary(int device, int which, int exp_lo, int exp_hi, uint64_t *n_tested, uint64_t *n_bad,
                             uint32_t bad_bits[16]);

/* 1 when this build's specular pipeline (shader.rs:472-543, the only one that calls powf) returns
 * the host C library's powf bit for bit -- the library was built against a glibc whose powf
 * tables it could read (csrc/gen_powf_tables.py); 0: the device library's powf, within 1 ulp. */
int tr_specular_exact(void);

/* shader.rs:97-112 registry */
int tr_pipeline_count(void);
const char *tr_pipeline_name(int i);

/* shader.rs:183-279 prepares, host-side (no GPU needed).  kind: 0 default_prepare,
 * 1 shadow_pass_prepare_1, 2 shadow_pass_prepare_2.  Matrices column-major (nalgebra). */
typedef struct tr_uniforms {
    float camera_direction[3];
    float t_light_direction[3];
    float vpmv[16];
    float i_vpmv[16];
    float m[16];
    float i_m[16];
    float it_m[16];
    float shadow_matrix[16];
} tr_uniforms;
int tr_prepare_uniforms(int kind, tr_uniforms *u, uint32_t width, uint32_t height,
                        const float light[3], const float look_from[3],
                        const float look_at[3], const float up[3]);
/* Host only: n model-space points (xyz: 3 n floats) through u->vpmv with the arithmetic, in the order, of the draw
 * chain's vertex transform (store_vertex_transformation_results, shader.rs:150-165): the matrix product column by
 * column, the homogeneous divide, then `as i32` of x and y (truncating, saturating).  xy[2 k], xy[2 k + 1] and z[k] are
 * therefore the pixel and the depth the renderer gives a mesh vertex at that point: endpoints for a tr_line.  ok[k] = 0
 * (and xy, z of it 0) where w is 0, a coordinate leaves +-2^20 or z is not finite within 2^100 -- what
 * tr_scene_set_lines would refuse --, else 1. */
int tr_project_points(const tr_uniforms *u, uint32_t n, const float *xyz, int32_t *xy, float *z, uint8_t *ok);
/* Host only: tr_projector_params.m = projector->vpmv * view->i_vpmv, the matrix that takes the raster of the frame's camera to the raster of
 * the projector's camera -- two ordinary tr_prepare_uniforms calls, at W x H and at pw x ph; the view's with kind 2,
 * which fills i_vpmv beside the same vpmv as kind 0 (an all-zero i_vpmv is refused).  Entry (r, c) is
 * ((P(r,0) V(0,c) + P(r,1) V(1,c)) + P(r,2) V(2,c)) + P(r,3) V(3,c) in double, rounded to f32 once. */
int tr_projector_matrix(const tr_uniforms *view, const tr_uniforms *projector, float m[16]);

/* Asset loading (app.rs:87-131): obj-rs `parse_obj` and image `open(..).into_rgb8()`
 * counterparts.  Returned objects are owned by the library; free with the matching call. */
int tr_load_obj(const char *path, tr_mesh **out);
void tr_free_mesh(tr_mesh *m);
int tr_load_tga_rgb8(const char *path, tr_image_rgb8 *out);
void tr_free_image(tr_image_rgb8 *img);
/* Frame writer (no counterpart upstream: the reference shows frames in a window): uncompressed
 * 24-bit TGA, top-left origin, i.e. exactly what tr_scene_get_frame_buffer returns. */
int tr_save_tga_rgb8(const char *path, const uint8_t *rgb, uint32_t w, uint32_t h);
/* The same frame as an 8-bit RGB PNG (stored deflate blocks: no compression library needed). */
int tr_save_png_rgb8(const char *path, const uint8_t *rgb, uint32_t w, uint32_t h);

const char *tr_last_error(void);
int tr_abi_version(void);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif
