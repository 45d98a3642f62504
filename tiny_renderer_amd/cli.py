"""Headless counterpart of the reference's CLI (src/main.rs:9-39: `-p <asset dir>`, `-s <pipeline>`).

The reference opens a window and orbits with the keyboard; here the camera / light angles are
explicit and the last frame is written as PNG, TGA or binary PPM.  Rendering happens on the GPU
through the C ABI.  `--gpus N` shards every frame by screen rows over N GPUs of the node (one
process per GPU, started from here; RCCL all-gather of the frame buffer, sharded.py).
"""
import argparse
import os
import sys
import time

import numpy as np


class _Once(argparse.Action):
    """An integer option that may be given at most once."""

    def __call__(self, parser, namespace, values, option_string=None):
        if getattr(namespace, self.dest, None) is not None:
            parser.error("%s may be given at most once" % option_string)
        setattr(namespace, self.dest, values)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="tiny_renderer_amd", description=__doc__)
    ap.add_argument("-p", dest="asset_path", default="assets/diablo", help="asset folder (main.rs:12)")
    ap.add_argument("-s", dest="pipeline", default="default", help="shader pipeline (main.rs:13)")
    ap.add_argument("--width", type=int, default=800)    # main.rs:6
    ap.add_argument("--height", type=int, default=800)   # main.rs:7
    ap.add_argument("--camera-angle", type=float, default=0.0, help="app.rs:158, radians")
    ap.add_argument("--light-angle", type=float, default=0.0, help="app.rs:159, radians")
    ap.add_argument("--frames", type=int, default=1, help="frames to render (camera orbits 2*pi over them)")
    ap.add_argument("--seconds", type=float, default=0.0,
                    help="run the reference's time-based frame loop for this long instead (app.rs:166-247): the "
                         "camera turns at CAMERA_SPEED = 3 rad/s as if a key were held, `FPS --- n` every second")
    ap.add_argument("--no-readback", action="store_true",
                    help="with --seconds: leave the frames on the GPU (the reference hands every frame to its window)")
    ap.add_argument("--out", default=None, help="write the last frame: .png, .tga (24-bit) or binary PPM otherwise; NAME.y4m: write "
                                                "EVERY frame of a --frames N run, in order, as YCbCr planes converted on the GPU (Scene.to_yuv_into; "
                                                "after every other stage option, behind --out-size or --ssaa)")
    ap.add_argument("--fps", type=int, default=30, metavar="N", help="the frame rate written into a .y4m file (default 30)")
    ap.add_argument("--yuv-matrix", default="bt709", choices=("bt601", "bt709"), help="the matrix of a .y4m file (default bt709)")
    ap.add_argument("--yuv-range", default="limited", choices=("full", "limited"), help="the range of a .y4m file (default limited)")
    ap.add_argument("--yuv-layout", default="i420", choices=("i420", "i444"), help="the planes of a .y4m file: i420 (C420jpeg; default) or i444 (C444)")
    ap.add_argument("--view", choices=("frame", "z", "shadow"), default="frame")  # app.rs:213-215
    ap.add_argument("--device", type=int, default=-1)
    ap.add_argument("--synthetic", action="store_true", help="procedural scene instead of -p")
    ap.add_argument("--gpus", type=int, default=1, help="shard every frame by screen rows over this many GPUs")
    ap.add_argument("--exchange", choices=("torch", "rccl", "peer", "peer-sparse"), default="torch",
                    help="--gpus N: how the bands travel (ShardedScene): torch = RCCL all-gather through torch.distributed, rccl = "
                         "the library's own RCCL communicator, peer / peer-sparse = the library's peer transport (these two also "
                         "run with several ranks on one GPU)")
    ap.add_argument("--instances", type=int, default=1,
                    help="draw the model N x N times, scaled by 1/N on a grid (instanced rendering; 1 = the model itself)")
    ap.add_argument("--instance-yaw", type=float, default=None, metavar="DEG",
                    help="with --instances N: turn grid cell (i, j) by (i * N + j) * DEG degrees about y (instance transforms; "
                         "placed and scaled as --instances alone places them)")
    ap.add_argument("--ssaa", type=int, default=1, choices=(1, 2, 4, 8),
                    help="supersampling: render at F * width x F * height and write the width x height picture, each pixel "
                         "the rounded mean of its F x F samples (resolved on the GPU: Scene.resolve)")
    ap.add_argument("--morph-to", default=None, metavar="OBJ",
                    help="a second OBJ of the model's topology: one morph target (its positions and normals minus the "
                         "model's), drawn at --morph-weight; with --frames N the weight runs a triangle wave between 0 and it")
    ap.add_argument("--morph-weight", type=float, default=1.0, metavar="W", help="weight of the --morph-to target (default 1)")
    ap.add_argument("--bend", type=float, default=None, metavar="DEG",
                    help="skinning with a procedural two-bone rig: weights follow a smooth step in model height, the upper "
                         "bone is turned about z by DEG degrees; with --frames N the angle ramps from 0 to DEG over the call")
    ap.add_argument("--with", dest="with_path", default=None, metavar="DIR",
                    help="a second asset folder: its model is rendered by a scene of its own -- own textures, same size, camera "
                         "and light -- and merged into the picture by depth on the GPU (Scene.composite)")
    ap.add_argument("--with-shader", default=None, metavar="PIPELINE", help="shader pipeline of the --with model (default: -s)")
    ap.add_argument("--with-offset", default="0,0,0", metavar="X,Y,Z", help="where the --with model stands (an instance offset)")
    ap.add_argument("--paint-with", dest="paint_path", default=None, metavar="DIR",
                    help="render the model of this asset folder at the size of the main model's diffuse texture and use that "
                         "frame as the texture (on the device: tr_scene_set_texture_from_frame) before the main render")
    ap.add_argument("--paint-shader", default=None, metavar="PIPELINE", help="shader pipeline of the --paint-with model (default: -s)")
    ap.add_argument("--shared-shadows", action="store_true",
                    help="with --with, both models on `shadow` or `occlusion`: render the light-space passes first, merge the "
                         "two shadow buffers on the GPU (Scene.shadow_merge), then the colour passes -- the models shade each "
                         "other as one scene of both would (needs --frames 1)")
    ap.add_argument("--ao", type=int, default=0, metavar="RADIUS",
                    help="screen-space ambient occlusion: darken the picture from its own z buffer on the GPU, samples on "
                         "rings of up to RADIUS (1..16) pixels (Scene.ambient_occlusion; after --with, before --ssaa resolves)")
    ap.add_argument("--ao-rings", type=int, default=1, metavar="N", help="rings of sixteen samples (1..4, at most RADIUS)")
    ap.add_argument("--ao-grey", action="store_true", help="with --ao: the occlusion alone, white darkened to black")
    ap.add_argument("--shutter", type=int, default=0, metavar="N",
                    help="motion blur: the written frame is the average of the last N (1..32) frames of the run, made on "
                         "the GPU (Scene.accumulate_in_place; needs --frames >= N; before --ssaa resolves)")
    ap.add_argument("--dof-focus", type=float, default=None, metavar="Z",
                    help="depth of field: blur the picture by its own z buffer on the GPU, the depth Z (the units of the z "
                         "buffer) stays sharp (Scene.depth_of_field; needs --dof-scale; after --with, --ao and --shutter, "
                         "before --ssaa resolves)")
    ap.add_argument("--dof-scale", type=float, default=None, metavar="S", help="pixels of blur radius per unit of z away from the sharp band")
    ap.add_argument("--dof-radius", type=int, default=4, metavar="R", help="largest blur radius in pixels (1..8, default 4)")
    ap.add_argument("--dof-range", type=float, default=0.0, metavar="B", help="half-width of the band of z around Z that stays sharp (default 0)")
    ap.add_argument("--dof-background", type=int, default=0, metavar="R", help="blur radius of pixels that are not drawn (0..--dof-radius, default 0)")
    ap.add_argument("--dof-show-coc", action="store_true", help="with --dof-focus: the blur radius of every pixel as a grey picture")
    ap.add_argument("--bloom", type=int, default=0, metavar="R",
                    help="bloom: the picture's highlights blurred by a tent of R (1..15) pixels and added back on the GPU "
                         "(Scene.bloom; after --with, --ao, --shutter and --dof-*, before --ssaa resolves)")
    ap.add_argument("--bloom-threshold", type=int, default=200, metavar="T", help="pixels whose largest channel exceeds T (0..255, default 200) glow")
    ap.add_argument("--bloom-strength", type=int, default=256, metavar="S", help="the glow is added scaled by S / 256 (0..1024, default 256)")
    ap.add_argument("--bloom-glow-only", action="store_true", help="with --bloom: the blurred highlights alone (threshold 0: the tent blur of the picture)")
    ap.add_argument("--lut", default=None, metavar="FILE.cube",
                    help="colour grading: the picture mapped through the 3-D lookup table of a .cube file (2..33 entries an axis, "
                         "unit domain) on the GPU (Scene.grade; after --bloom, before --ssaa resolves)")
    ap.add_argument("--gamma", type=float, default=None, metavar="G",
                    help="colour grading by a 33^3 table of v^(1/G), e.g. 2.2 (Scene.grade; after --bloom, before --ssaa resolves)")
    ap.add_argument("--outline", type=int, default=None, metavar="R",
                    help="outlines: ink on the picture's silhouettes and depth steps, found in its own z buffer on the GPU, reaching "
                         "R (0..3) pixels from the edge (Scene.outline; after --lut / --gamma / --auto-levels, so the table does not "
                         "recolour the ink, and before --ssaa resolves, so supersampling smooths the lines)")
    ap.add_argument("--outline-depth", type=float, default=4.0, metavar="T",
                    help="a drawn neighbour more than T units of z farther away makes a depth step (default 4)")
    ap.add_argument("--outline-crease", type=float, default=None, metavar="T",
                    help="also ink folds: pixels whose second difference of z along a row or a column exceeds T")
    ap.add_argument("--outline-colour", default="0,0,0", metavar="r,g,b", help="the ink (default 0,0,0)")
    ap.add_argument("--outline-opacity", type=int, default=256, metavar="N", help="the ink covers N / 256 of the picture (0..256, default 256)")
    ap.add_argument("--outline-only", action="store_true", help="with --outline: the lines alone, on white paper")
    ap.add_argument("--wireframe", nargs="?", const="255,255,255", default=None, metavar="R,G,B[,A]",
                    help="lines: the mesh's edges drawn over the frame on the GPU, hidden behind the model by the frame's own depth "
                         "(Scene.set_lines through wireframe_lines, Scene.lines; after --outline, before --aa, which smooths them)")
    ap.add_argument("--wire-width", type=int, default=1, metavar="N", help="with --wireframe: the lines' width in pixels, 1..15 (default 1)")
    ap.add_argument("--wire-bias", type=float, default=0.5, metavar="F",
                    help="with --wireframe: added to the lines' depth before the test; nearer is larger, so a positive bias lifts an "
                         "edge off its own surface (default 0.5: DESIGN.md 7za has the sweep it was chosen on)")
    ap.add_argument("--wire-xray", action="store_true", help="with --wireframe: no depth test, the far side shows through")
    ap.add_argument("--wire-only", action="store_true", help="with --wireframe: clear the frame, then draw the lines alone (no depth test)")
    ap.add_argument("--glow", default=None, metavar="R,G,B[,A]",
                    help="distance field: a glow of that colour around the model, added on the GPU and gone --glow-radius pixels away "
                         "(Scene.distance_ramp through ramp_glow; keeps the model; after --wireframe, before --aa)")
    ap.add_argument("--glow-radius", type=int, default=24, metavar="N", help="with --glow and --inner-glow: the reach in pixels, 1..255 (default 24)")
    ap.add_argument("--stroke", default=None, metavar="R,G,B[,A]",
                    help="distance field: a stroke of that colour around the model's silhouette (Scene.distance_ramp through ramp_stroke; "
                         "keeps the model; after --glow, before --aa)")
    ap.add_argument("--stroke-width", type=int, default=4, metavar="N", help="with --stroke: the width in pixels, 1..254 (default 4)")
    ap.add_argument("--inner-glow", default=None, metavar="R,G,B[,A]",
                    help="distance field: a glow of that colour inside the model along its silhouette (TR_DIST_INVERT: the seeds are "
                         "the pixels where nothing is drawn, and they are kept; before --glow)")
    ap.add_argument("--aa", action="store_true",
                    help="edge anti-aliasing: smooth the picture's stair-steps at its own size by a luma-driven edge filter on the GPU "
                         "(Scene.antialias; after --outline, so the ink's edges are smoothed too, and before --ssaa resolves)")
    ap.add_argument("--aa-contrast", default="8,32", metavar="MIN,REL",
                    help="filter a pixel whose local luma range reaches MIN (0..255) and REL / 256 (0..256) of the brightest luma (default 8,32)")
    ap.add_argument("--aa-search", type=int, default=8, metavar="N", help="look for an edge's ends up to N pixels away (1..8, default 8)")
    ap.add_argument("--aa-subpixel", type=int, default=192, metavar="N", help="the weight of the sub-pixel term (0..256, default 192; 0: edges only)")
    ap.add_argument("--aa-show-blend", action="store_true", help="with --aa: the blend weight the filter found instead of the picture")
    ap.add_argument("--rotate", type=float, default=None, metavar="DEG",
                    help="warp: turn the picture counter-clockwise by DEG degrees about its centre on the GPU (Scene.warp through "
                         "warp_grid_rotate; after --aa and before --out-size)")
    ap.add_argument("--lens", default=None, metavar="K1[,K2]",
                    help="warp: a Brown-Conrady radial lens, r -> r (1 + K1 r^2 + K2 r^4) with r = 1 at the corner (warp_grid_lens; "
                         "K1 < 0 barrel, K1 > 0 pincushion); applied after --rotate")
    ap.add_argument("--chromatic", type=float, default=None, metavar="PX",
                    help="warp: scale red and blue apart radially, PX pixels at the corner (warp_grid_chromatic: a grid a channel); "
                         "applied after --lens")
    ap.add_argument("--warp-edge", default=None, choices=("border", "clamp"),
                    help="what --rotate, --lens and --chromatic show outside the picture: black (border; default) or its nearest pixel (clamp)")
    ap.add_argument("--blur", type=float, default=None, metavar="SIGMA",
                    help="convolve: a separable Gaussian blur of SIGMA pixels, clamped at the edge, on the GPU (Scene.convolve "
                         "through kernel_gaussian; after the warp options and before --out-size)")
    ap.add_argument("--sharpen", default=None, metavar="AMOUNT[,SIGMA]",
                    help="convolve: an unsharp mask, picture + AMOUNT * (picture - its Gaussian blur of SIGMA pixels, default 1.5); "
                         "AMOUNT 0..4; applied after --blur")
    ap.add_argument("--emboss", action="store_true", help="convolve: a 3 x 3 emboss around mid grey (kernel_emboss, bias 128); applied after --sharpen")
    ap.add_argument("--edges", action="store_true", help="convolve: the absolute 3 x 3 Laplacian (kernel_laplacian); applied after --emboss")
    ap.add_argument("--convolve", default=None, metavar="ROWS",
                    help='convolve: a kernel of integer weights, rows from the top separated by ";", weights by ",": '
                         '"0,-1,0;-1,5,-1;0,-1,0" (odd sides up to 9; black outside the picture); applied after --edges')
    ap.add_argument("--convolve-shift", type=int, default=0, metavar="N", help="with --convolve: shift the sum right by N bits, rounded (0..22)")
    ap.add_argument("--convolve-bias", type=int, default=0, metavar="N", help="with --convolve: add N afterwards (-255..255)")
    ap.add_argument("--erode", type=int, default=None, action=_Once, metavar="N",
                    help="rank: the minimum over a footprint of radius N (1..7), clamped at the edge, on the GPU (Scene.rank; after "
                         "the convolve options and before --overlay)")
    ap.add_argument("--dilate", type=int, default=None, action=_Once, metavar="N", help="rank: the maximum over a footprint of radius N (1..7); applied after --erode")
    ap.add_argument("--median", type=int, default=None, action=_Once, metavar="N", help="rank: the median over a footprint of radius N (1..7); applied after --dilate")
    ap.add_argument("--despeckle", type=int, default=None, action=_Once, metavar="N",
                    help="rank: every pixel clamped between the second lowest and the second highest value of its footprint of radius N "
                         "(1..7); applied after --median")
    ap.add_argument("--rank-shape", default=None, choices=("rect", "disc", "cross"),
                    help="the footprint of --erode, --dilate, --median and --despeckle: the whole square (rect; default), a disc or a cross")
    ap.add_argument("--smooth", type=int, default=None, action=_Once, metavar="R",
                    help="bilateral: edge-preserving smoothing over a box of radius R (1..7), clamped at the edge, on the GPU "
                         "(Scene.bilateral; after the rank options and before --overlay)")
    ap.add_argument("--smooth-range", type=int, default=None, action=_Once, metavar="N",
                    help="with --smooth or --ao-smooth: only taps within N (0..255) of the centre count, all alike (range_step; default 16)")
    ap.add_argument("--smooth-guide", default=None, choices=("colour", "depth"),
                    help="with --smooth: the distance is the largest channel difference (colour; default) or the depth difference times "
                         "--smooth-depth-scale (depth)")
    ap.add_argument("--smooth-depth-scale", type=float, default=None, action=_Once, metavar="F",
                    help="with --smooth-guide depth or --ao-smooth: distance steps per unit of depth (finite, >= 0; default 8)")
    ap.add_argument("--ao-smooth", type=int, default=None, action=_Once, metavar="R",
                    help="with --ao: the depth-guided bilateral blur over a box of radius R (1..7) directly behind the occlusion -- "
                         "its grain goes, the silhouettes stay")
    ap.add_argument("--backdrop", default=None, metavar="FILE.tga|R,G,B[:R,G,B]",
                    help="layer: a picture, a colour or a gradient from the top colour to the bottom one behind the model, blended "
                         "on the GPU where nothing is drawn (Scene.layer, where=\"undrawn\"; after --with and --ao, before the "
                         "depth-of-field and bloom options)")
    ap.add_argument("--projector", default=None, metavar="FILE.tga",
                    help="projector: cast that image onto the model on the GPU from a second camera at --projector-from looking at "
                         "--projector-at, a slide projector or a light cookie (after --with, --ao and --backdrop, before --fog and the depth views)")
    ap.add_argument("--projector-from", default="1.5,1.0,1.5", metavar="X,Y,Z", help="with --projector: where the projector stands (default 1.5,1.0,1.5)")
    ap.add_argument("--projector-at", default="0,0,0", metavar="X,Y,Z", help="with --projector: what it looks at (default 0,0,0; up is the camera's)")
    ap.add_argument("--projector-mode", default="add", choices=("normal", "add", "multiply", "screen", "lighten", "darken", "difference"),
                    help="with --projector: how the image is blended into the frame (default add: light)")
    ap.add_argument("--projector-opacity", type=int, default=256, metavar="N", help="with --projector: 0..256 (default 256)")
    ap.add_argument("--projector-shadows", action="store_true",
                    help="with --projector: the model shadows the projected light -- a second scene of the same mesh, of the image's size, is "
                         "rendered from the projector and its depth is the shadow map")
    ap.add_argument("--projector-bias", type=float, default=2.0, metavar="F",
                    help="with --projector-shadows: added to a pixel's depth before the shadow test (nearer is larger; default 2)")
    ap.add_argument("--projector-soft", action="store_true", help="with --projector-shadows: filter the shadow's edge over 2 x 2 texels")
    ap.add_argument("--light-point", action="append", default=[], metavar="X,Y,Z:R,G,B[:INTENSITY[:FALLOFF]]",
                    help="relight: a coloured point light at X,Y,Z (model space) laid on the frame on the GPU from normals recovered out of "
                         "its depth (Scene.relight; repeatable, at most 8 lights in all; after --projector, before --fog; write a value that begins "
                         "with a minus sign as --light-point=-1,2,3:..)")
    ap.add_argument("--light-spot", action="append", default=[], metavar="X,Y,Z:AX,AY,AZ:R,G,B:INNER,OUTER[:INTENSITY[:FALLOFF]]",
                    help="relight: a spot light at X,Y,Z shining at AX,AY,AZ, full inside INNER degrees, none outside OUTER (repeatable)")
    ap.add_argument("--light-dir", action="append", default=[], metavar="X,Y,Z:R,G,B[:INTENSITY]",
                    help="relight: a directional light; X,Y,Z points towards it (repeatable)")
    ap.add_argument("--light-ambient", default=None, metavar="R,G,B", help="relight: the ambient term (default 0,0,0)")
    ap.add_argument("--light-mode", default="add", choices=("normal", "add", "multiply", "screen", "lighten", "darken", "difference"),
                    help="relight: how the light is blended into the frame (default add)")
    ap.add_argument("--light-albedo", default=None, choices=("on", "off"),
                    help="relight: multiply the light by the pixel's own colour first (default: on with --light-mode add, off otherwise)")
    ap.add_argument("--light-specular", default=None, metavar="S,K", help="relight: a highlight of strength S and exponent 2^K (K 0..10) on every light")
    ap.add_argument("--show-normals", action="store_true", help="relight: the normal map recovered from the depth instead of the lights")
    ap.add_argument("--fog", default=None, metavar="R,G,B",
                    help="depth ramp: fog of that colour, thickening with distance, blended into the model on the GPU (Scene.ramp "
                         "through ramp_fog; after --with, --ao and --backdrop, before the depth-of-field and bloom options)")
    ap.add_argument("--fog-kind", default="linear", choices=("linear", "exp", "exp2"), help="with --fog: the falloff (default linear)")
    ap.add_argument("--fog-density", type=float, default=2.0, metavar="D", help="with --fog and an exponential --fog-kind: the density (default 2)")
    ap.add_argument("--fog-span", default="auto", metavar="NEAR,FAR|auto",
                    help="with --fog, --depth-view and --depth-contours: the depths where the ramp starts and where it ends (nearer is "
                         "larger), or auto: the nearest and farthest drawn depth, found on the GPU (ramp_span_auto; default)")
    ap.add_argument("--fog-background", action="store_true", help="with --fog: fog out the pixels where nothing is drawn, too")
    ap.add_argument("--depth-view", default=None, choices=("grey", "colour"),
                    help="depth ramp: the model coloured by its depth, white (near) to black or through false colours (Scene.ramp "
                         "through ramp_grey / ramp_false_colour; in the place of --fog's, before it)")
    ap.add_argument("--depth-contours", type=int, default=None, metavar="N",
                    help="depth ramp: N black contour bands over the span (1..128; ramp_contours; after --depth-view, before --fog)")
    ap.add_argument("--overlay", default=None, metavar="FILE.tga",
                    help="layer: a picture blended over the finished frame on the GPU (Scene.layer; after the convolve options, "
                         "before --vignette, --out-size and y4m output)")
    ap.add_argument("--overlay-at", default="0,0", metavar="X,Y", help="with --overlay: where its top-left pixel lands (signed; default 0,0)")
    ap.add_argument("--overlay-opacity", type=int, default=256, metavar="N", help="with --overlay: 0..256 (default 256, opaque)")
    ap.add_argument("--overlay-mode", default="normal", choices=("normal", "add", "multiply", "screen", "lighten", "darken", "difference"),
                    help="with --overlay: the blend (default normal)")
    ap.add_argument("--vignette", type=int, default=None, metavar="N",
                    help="layer: darken the picture towards its corners by up to N of 255 (layer_vignette multiplied in; after --overlay)")
    ap.add_argument("--out-size", default=None, metavar="WxH",
                    help="resize: write the picture scaled to W x H (each 1..8192 and at least an eighth of the rendered side) on "
                         "the GPU (Scene.resize; applied last, after --aa, in the place of the --ssaa resolve)")
    ap.add_argument("--resize-filter", default="area", choices=("area", "bilinear"),
                    help="the filter of --out-size: area (pixel overlap; default) or bilinear (a triangle that widens when shrinking)")
    ap.add_argument("--auto-levels", default=None, metavar="LOW,HIGH",
                    help="colour grading by a table made from the picture itself: its luma percentiles LOW and HIGH (e.g. 0.01,0.99), "
                         "found on the GPU (Scene.get_frame_stats), stretched to black and white (lut_auto_levels; in the place of "
                         "--lut / --gamma)")
    ap.add_argument("--dof-autofocus", action="store_true",
                    help="depth of field focused on the median depth of what is drawn in the central quarter of the picture "
                         "(depth_median; in the place of --dof-focus Z, with --dof-scale S)")
    ap.add_argument("--stats", action="store_true",
                    help="print the finished picture's statistics (Scene.get_frame_stats): pixels, drawn pixels, depth range, the "
                         "box of what is drawn and the luma bins at 1, 50 and 99 %%")
    args = ap.parse_args(argv)
    args.grade_lut = None
    args.levels = None
    if sum(v is not None for v in (args.lut, args.gamma, args.auto_levels)) > 1:
        ap.error("--lut, --gamma and --auto-levels are tables for one stage: give one")
    if args.auto_levels is not None or args.stats or args.dof_autofocus:
        if args.gpus > 1 or args.seconds > 0 or args.view != "frame":
            ap.error("--auto-levels, --dof-autofocus and --stats work on the frame of one GPU, by frame count: use --gpus 1, --frames and --view frame")
    if args.auto_levels is not None:
        try:
            low, high = (float(v) for v in args.auto_levels.split(","))
            if not 0.0 <= low < high <= 1.0:
                raise ValueError
        except ValueError:
            ap.error("--auto-levels takes LOW,HIGH with 0 <= LOW < HIGH <= 1")
        args.levels = (low, high)
    if args.lut is not None or args.gamma is not None:
        if args.gpus > 1 or args.seconds > 0 or args.view != "frame":
            ap.error("--lut and --gamma work on the colour frame of one GPU, by frame count: use --gpus 1, --frames and --view frame")
        from .scene import load_cube, lut_from_function
        try:
            if args.lut is not None:
                args.grade_lut = load_cube(args.lut)
            else:
                if not args.gamma > 0.0:
                    raise ValueError("--gamma must be positive")
                args.grade_lut = lut_from_function(33, lambda v: v ** (1.0 / args.gamma))
        except (OSError, ValueError) as e:
            ap.error(str(e))
    args.backdrop_spec = None
    if args.overlay is None and (args.overlay_at != "0,0" or args.overlay_opacity != 256 or args.overlay_mode != "normal"):
        ap.error("--overlay-at, --overlay-opacity and --overlay-mode go with --overlay FILE.tga")
    if args.backdrop is not None or args.overlay is not None or args.vignette is not None:
        if args.gpus > 1 or args.seconds > 0 or args.view != "frame":
            ap.error("--backdrop, --overlay and --vignette work on the colour frame of one GPU, by frame count: use --gpus 1, --frames and --view frame")
        try:
            if args.backdrop is not None:
                if args.backdrop.lower().endswith(".tga"):
                    args.backdrop_spec = args.backdrop
                else:
                    ends = [tuple(int(v) for v in c.split(",")) for c in args.backdrop.split(":")]
                    if not 1 <= len(ends) <= 2 or any(len(c) != 3 or min(c) < 0 or max(c) > 255 for c in ends):
                        raise ValueError("--backdrop takes FILE.tga, R,G,B or R,G,B:R,G,B with values 0..255")
                    args.backdrop_spec = (ends[0], ends[-1])
            if args.overlay is not None:
                at = [int(v) for v in args.overlay_at.split(",")]
                if len(at) != 2 or not 0 <= args.overlay_opacity <= 256:
                    raise ValueError("--overlay-at takes X,Y and --overlay-opacity 0..256")
                args.overlay_at = at
            if args.vignette is not None and not 0 <= args.vignette <= 255:
                raise ValueError("--vignette takes 0..255")
        except ValueError as e:
            ap.error(str(e))
    args.projector_view = None
    if args.projector is None and (args.projector_from != "1.5,1.0,1.5" or args.projector_at != "0,0,0" or args.projector_mode != "add"
                                   or args.projector_opacity != 256 or args.projector_shadows or args.projector_bias != 2.0 or args.projector_soft):
        ap.error("--projector-from, -at, -mode, -opacity, -shadows, -bias and -soft go with --projector FILE.tga")
    if args.projector is not None:
        if args.gpus > 1 or args.seconds > 0 or args.view != "frame":
            ap.error("--projector works on the frame of one GPU, by frame count: use --gpus 1, --frames and --view frame")
        try:
            view = [[float(v) for v in t.split(",")] for t in (args.projector_from, args.projector_at)]
            if len(view[0]) != 3 or len(view[1]) != 3 or view[0] == view[1]:
                raise ValueError("--projector-from and --projector-at take X,Y,Z, two different points")
            if not 0 <= args.projector_opacity <= 256:
                raise ValueError("--projector-opacity takes 0..256")
            if not np.isfinite(np.float32(args.projector_bias)):
                raise ValueError("--projector-bias must be finite")
            if (args.projector_soft or args.projector_bias != 2.0) and not args.projector_shadows:
                raise ValueError("--projector-bias and --projector-soft go with --projector-shadows")
            args.projector_view = view
        except ValueError as e:
            ap.error(str(e))
    args.relight = None
    wants_light = bool(args.light_point or args.light_spot or args.light_dir or args.show_normals or args.light_ambient is not None)
    if not wants_light and (args.light_mode != "add" or args.light_albedo is not None or args.light_specular is not None):
        ap.error("--light-mode, --light-albedo and --light-specular go with --light-point, --light-spot, --light-dir, --light-ambient or --show-normals")
    if wants_light:
        if args.gpus > 1 or args.seconds > 0 or args.view != "frame":
            ap.error("the --light options work on the frame of one GPU, by frame count: use --gpus 1, --frames and --view frame")
        try:
            args.relight = _parse_lights(args)
        except ValueError as e:
            ap.error(str(e))
    args.fog_colour = None
    if args.fog is None and (args.fog_kind != "linear" or args.fog_density != 2.0 or args.fog_background):
        ap.error("--fog-kind, --fog-density and --fog-background go with --fog R,G,B")
    if args.fog is None and args.depth_view is None and args.depth_contours is None and args.fog_span != "auto":
        ap.error("--fog-span goes with --fog, --depth-view or --depth-contours")
    if args.fog is not None or args.depth_view is not None or args.depth_contours is not None:
        if args.gpus > 1 or args.seconds > 0 or args.view != "frame":
            ap.error("--fog, --depth-view and --depth-contours work on the frame of one GPU, by frame count: use --gpus 1, --frames and --view frame")
        try:
            if args.fog is not None:
                args.fog_colour = tuple(int(v) for v in args.fog.split(","))
                if len(args.fog_colour) != 3 or min(args.fog_colour) < 0 or max(args.fog_colour) > 255:
                    raise ValueError("--fog takes R,G,B with values 0..255")
                if not args.fog_density > 0.0:
                    raise ValueError("--fog-density must be positive")
            if args.depth_contours is not None and not 1 <= args.depth_contours <= 128:
                raise ValueError("--depth-contours takes 1..128")
            if args.fog_span != "auto":
                span = [float(v) for v in args.fog_span.split(",")]
                if len(span) != 2 or span[0] == span[1]:
                    raise ValueError("--fog-span takes NEAR,FAR (two different depths) or auto")
                args.fog_span = span
        except ValueError as e:
            ap.error(str(e))
    args.outline_params = None
    if args.outline is None and (args.outline_depth != 4.0 or args.outline_crease is not None or args.outline_colour != "0,0,0"
                                 or args.outline_opacity != 256 or args.outline_only):
        ap.error("--outline-depth, --outline-crease, --outline-colour, --outline-opacity and --outline-only go with --outline R")
    if args.outline is not None:
        if args.gpus > 1 or args.seconds > 0 or args.view != "frame":
            ap.error("--outline works on the colour frame of one GPU, by frame count: use --gpus 1, --frames and --view frame")
        from .scene import outline_params
        try:
            ink = [int(v) for v in args.outline_colour.split(",")]
            args.outline_params = outline_params(args.outline, depth_step=args.outline_depth, crease=args.outline_crease, ink=ink,
                                                 opacity=args.outline_opacity, only=args.outline_only)
        except ValueError as e:
            ap.error(str(e))
    args.wire_colour = None
    if args.wireframe is None and (args.wire_width != 1 or args.wire_bias != 0.5 or args.wire_xray or args.wire_only):
        ap.error("--wire-width, --wire-bias, --wire-xray and --wire-only go with --wireframe")
    if args.wireframe is not None:
        if args.gpus > 1 or args.seconds > 0 or args.view != "frame" or args.frames != 1 or args.shutter:
            ap.error("--wireframe draws over one frame of one GPU under its camera: use --gpus 1, --frames 1 and --view frame")
        try:
            args.wire_colour = tuple(int(v) for v in args.wireframe.split(","))
            if len(args.wire_colour) not in (3, 4) or min(args.wire_colour) < 0 or max(args.wire_colour) > 255:
                raise ValueError("--wireframe takes R,G,B[,A] with values 0..255")
            if not 1 <= args.wire_width <= 15:
                raise ValueError("--wire-width takes 1..15")
            if not np.isfinite(np.float32(args.wire_bias)):
                raise ValueError("--wire-bias must be finite")
        except ValueError as e:
            ap.error(str(e))
    args.glow_colour = args.stroke_colour = args.inner_glow_colour = None
    if args.glow is None and args.inner_glow is None and args.glow_radius != 24:
        ap.error("--glow-radius goes with --glow or --inner-glow")
    if args.stroke is None and args.stroke_width != 4:
        ap.error("--stroke-width goes with --stroke")
    if args.glow is not None or args.stroke is not None or args.inner_glow is not None:
        if args.gpus > 1 or args.seconds > 0 or args.view != "frame":
            ap.error("--glow, --stroke and --inner-glow work on the frame of one GPU, by frame count: use --gpus 1, --frames and --view frame")
        try:
            for name in ("glow", "stroke", "inner_glow"):
                text = getattr(args, name)
                if text is not None:
                    colour = tuple(int(v) for v in text.split(","))
                    if len(colour) not in (3, 4) or min(colour) < 0 or max(colour) > 255:
                        raise ValueError("--%s takes R,G,B[,A] with values 0..255" % name.replace("_", "-"))
                    setattr(args, name + "_colour", colour)
            if not 1 <= args.glow_radius <= 255:
                raise ValueError("--glow-radius takes 1..255")
            if not 1 <= args.stroke_width <= 254:
                raise ValueError("--stroke-width takes 1..254")
        except ValueError as e:
            ap.error(str(e))
    args.aa_params = None
    if not args.aa and (args.aa_contrast != "8,32" or args.aa_search != 8 or args.aa_subpixel != 192 or args.aa_show_blend):
        ap.error("--aa-contrast, --aa-search, --aa-subpixel and --aa-show-blend go with --aa")
    if args.aa:
        if args.gpus > 1 or args.seconds > 0 or args.view != "frame":
            ap.error("--aa works on the colour frame of one GPU, by frame count: use --gpus 1, --frames and --view frame")
        from .scene import aa_params
        try:
            lo, rel = (int(v) for v in args.aa_contrast.split(","))
            args.aa_params = aa_params(contrast_min=lo, contrast_rel=rel, search=args.aa_search, subpixel=args.aa_subpixel,
                                       show_blend=args.aa_show_blend)
        except ValueError as e:
            ap.error(str(e))
    args.bloom_params = None
    if not args.bloom and (args.bloom_threshold != 200 or args.bloom_strength != 256 or args.bloom_glow_only):
        ap.error("--bloom-threshold, --bloom-strength and --bloom-glow-only go with --bloom R")
    if args.bloom:
        if args.gpus > 1 or args.seconds > 0 or args.view != "frame":
            ap.error("--bloom works on the colour frame of one GPU, by frame count: use --gpus 1, --frames and --view frame")
        from .scene import bloom_params
        try:
            args.bloom_params = bloom_params(args.bloom, threshold=args.bloom_threshold, strength=args.bloom_strength,
                                             flags=1 if args.bloom_glow_only else 0)
        except ValueError as e:
            ap.error(str(e))
    args.dof = None
    if args.dof_autofocus and args.dof_focus is not None:
        ap.error("--dof-autofocus finds the focus that --dof-focus Z states: give one")
    if args.dof_autofocus and args.dof_scale is None:
        ap.error("--dof-autofocus goes with --dof-scale S")
    if not args.dof_autofocus and (args.dof_focus is None) != (args.dof_scale is None):
        ap.error("--dof-focus Z and --dof-scale S go together")
    if args.dof_focus is None and not args.dof_autofocus and (args.dof_radius != 4 or args.dof_range != 0.0 or args.dof_background != 0 or args.dof_show_coc):
        ap.error("--dof-radius, --dof-range, --dof-background and --dof-show-coc go with --dof-focus Z --dof-scale S")
    if args.dof_autofocus:
        from .scene import dof_params
        try:   # (the focus is found at run time; everything else is checked now)
            dof_params(0.0, args.dof_scale, max_radius=args.dof_radius, background_radius=args.dof_background,
                       flags=1 if args.dof_show_coc else 0, range=args.dof_range)
        except ValueError as e:
            ap.error(str(e))
    if args.dof_focus is not None:
        if args.gpus > 1 or args.seconds > 0 or args.view != "frame":
            ap.error("--dof-focus blurs the colour frame of one GPU, by frame count: use --gpus 1, --frames and --view frame")
        from .scene import dof_params
        try:
            args.dof = dof_params(args.dof_focus, args.dof_scale, max_radius=args.dof_radius, background_radius=args.dof_background,
                                  flags=1 if args.dof_show_coc else 0, range=args.dof_range)
        except ValueError as e:
            ap.error(str(e))
    if args.shutter and not 1 <= args.shutter <= 32:
        ap.error("--shutter takes 1..32 frames")
    if args.shutter and (args.gpus > 1 or args.ao or args.with_path):
        ap.error("--shutter averages the frames of one scene on one GPU: not with --gpus > 1, --ao or --with")
    if args.shutter and (args.seconds > 0 or args.view != "frame" or args.frames < args.shutter):
        ap.error("--shutter N averages the last N colour frames of a run by frame count: use --frames >= N and --view frame")
    if (args.ao_rings != 1 or args.ao_grey) and not args.ao:
        ap.error("--ao-rings and --ao-grey go with --ao RADIUS")
    if args.ao and (args.gpus > 1 or args.seconds > 0 or args.view != "frame"):
        ap.error("--ao shades the colour frame of one GPU, by frame count: use --gpus 1, --frames and --view frame")
    if args.ao and not (1 <= args.ao <= 16 and 1 <= args.ao_rings <= min(4, args.ao)):
        ap.error("--ao takes a radius of 1..16 pixels, --ao-rings 1..4 and at most the radius")
    if args.with_path and (args.gpus > 1 or args.seconds > 0):
        ap.error("--with merges two scenes of one GPU, by frame count: use --gpus 1 and --frames")
    if args.with_path:
        try:
            args.with_offset = [float(v) for v in args.with_offset.split(",")]
            assert len(args.with_offset) == 3
        except (ValueError, AssertionError):
            ap.error("--with-offset takes three numbers: x,y,z")
    if args.shared_shadows:
        from .scene import TWO_PASS_PIPELINES
        if not args.with_path:
            ap.error("--shared-shadows goes with --with DIR")
        if args.pipeline not in TWO_PASS_PIPELINES or (args.with_shader or args.pipeline) not in TWO_PASS_PIPELINES:
            ap.error("--shared-shadows needs a shadow buffer on both sides: -s and --with-shader must be `shadow` or `occlusion`")
        if args.frames != 1 or args.shutter or args.seconds > 0 or args.gpus > 1:
            ap.error("--shared-shadows renders one frame of one GPU pass by pass: use --frames 1 and --gpus 1, without --shutter "
                     "and --seconds")
        # (--bend and --morph-to pose the first model as scene state: the one frame's passes draw that pose)
    if args.bend is not None and (args.gpus > 1 or args.seconds > 0 or args.morph_to):
        ap.error("--bend skins the scene of one GPU, by frame count, without --morph-to: use --gpus 1 and --frames")
    if args.morph_to and (args.gpus > 1 or args.seconds > 0):
        ap.error("--morph-to poses the scene of one GPU, by frame count: use --gpus 1 and --frames")
    if args.ssaa > 1 and (args.gpus > 1 or args.view != "frame"):
        ap.error("--ssaa resolves the colour frame of one GPU: use --gpus 1 and --view frame")
    args.warps = []
    if args.rotate is not None or args.lens is not None or args.chromatic is not None:
        if args.gpus > 1 or args.seconds > 0 or args.view != "frame":
            ap.error("--rotate, --lens and --chromatic work on the colour frame of one GPU, by frame count: use --gpus 1, --frames and --view frame")
        from .scene import warp_grid_rotate, warp_grid_lens, warp_grid_chromatic, warp_params
        edge = args.warp_edge or "border"
        if args.rotate is not None:
            args.warps.append((warp_grid_rotate(args.rotate, args.width, args.height), warp_params(edge)))
        if args.lens is not None:
            try:
                k = [float(v) for v in args.lens.split(",")]
                if not 1 <= len(k) <= 2:
                    raise ValueError
            except ValueError:
                ap.error("--lens takes one or two numbers: K1[,K2]")
            args.warps.append((warp_grid_lens(k[0], k[1] if len(k) > 1 else 0.0, args.width, args.height), warp_params(edge)))
        if args.chromatic is not None:
            args.warps.append((warp_grid_chromatic(args.chromatic, args.width, args.height), warp_params(edge, per_channel=True)))
    elif args.warp_edge is not None:
        ap.error("--warp-edge goes with --rotate, --lens or --chromatic")
    args.convolves = []
    if args.convolve is None and (args.convolve_shift or args.convolve_bias):
        ap.error("--convolve-shift and --convolve-bias go with --convolve")
    if args.blur is not None or args.sharpen is not None or args.emboss or args.edges or args.convolve is not None:
        if args.gpus > 1 or args.seconds > 0 or args.view != "frame":
            ap.error("--blur, --sharpen, --emboss, --edges and --convolve work on the colour frame of one GPU, by frame count: "
                     "use --gpus 1, --frames and --view frame")
        from .scene import convolve_params, kernel_gaussian, kernel_laplacian, kernel_emboss
        try:
            if args.blur is not None:
                k, shift = kernel_gaussian(args.blur)
                args.convolves.append(convolve_params(k, shift=shift, edge="clamp"))
            if args.sharpen is not None:
                v = [float(x) for x in args.sharpen.split(",")]
                if not 1 <= len(v) <= 2:
                    raise ValueError("--sharpen takes one or two numbers: AMOUNT[,SIGMA]")
                k, shift = kernel_gaussian(v[1] if len(v) > 1 else 1.5)
                args.convolves.append(convolve_params(k, shift=shift, edge="clamp", unsharp=int(round(256.0 * v[0]))))
            if args.emboss:
                args.convolves.append(convolve_params(kernel_emboss()[0], bias=128, edge="clamp"))
            if args.edges:
                args.convolves.append(convolve_params(kernel_laplacian()[0], edge="clamp", absolute=True))
            if args.convolve is not None:
                rows = [[int(x) for x in r.split(",")] for r in args.convolve.split(";")]
                if len(set(len(r) for r in rows)) != 1:
                    raise ValueError("--convolve: every row has the same number of weights")
                args.convolves.append(convolve_params(np.array(rows, np.int32), shift=args.convolve_shift, bias=args.convolve_bias))
        except ValueError as e:
            ap.error(str(e))
    args.ranks = []
    if all(v is None for v in (args.erode, args.dilate, args.median, args.despeckle)):
        if args.rank_shape is not None:
            ap.error("--rank-shape goes with --erode, --dilate, --median or --despeckle")
    else:
        if args.gpus > 1 or args.seconds > 0 or args.view != "frame":
            ap.error("--erode, --dilate, --median and --despeckle work on the colour frame of one GPU, by frame count: "
                     "use --gpus 1, --frames and --view frame")
        from .scene import rank_params, footprint_rect, footprint_disc, footprint_cross
        shape = {"rect": lambda r: footprint_rect(2 * r + 1, 2 * r + 1), "disc": footprint_disc, "cross": footprint_cross}[args.rank_shape or "rect"]
        for name, r in (("--erode", args.erode), ("--dilate", args.dilate), ("--median", args.median), ("--despeckle", args.despeckle)):
            if r is None:
                continue
            if not 1 <= r <= 7:
                ap.error(name + " takes a radius 1..7")
            f = shape(r)
            n = int(f.sum())
            if name == "--despeckle":
                args.ranks.append(rank_params(f, 1, n - 2, op="clamp_centre", edge="clamp"))
            else:
                args.ranks.append(rank_params(f, {"--erode": "min", "--dilate": "max", "--median": "median"}[name], edge="clamp"))
    args.smooths, args.ao_smooth_params = [], None
    if args.smooth is None and args.ao_smooth is None:
        if args.smooth_range is not None or args.smooth_guide is not None or args.smooth_depth_scale is not None:
            ap.error("--smooth-range, --smooth-guide and --smooth-depth-scale go with --smooth or --ao-smooth")
    else:
        if args.gpus > 1 or args.seconds > 0 or args.view != "frame":
            ap.error("--smooth and --ao-smooth work on the colour frame of one GPU, by frame count: use --gpus 1, --frames and --view frame")
        if args.ao_smooth is not None and not args.ao:
            ap.error("--ao-smooth goes with --ao RADIUS")
        if args.smooth is None and args.smooth_guide is not None:
            ap.error("--smooth-guide goes with --smooth (--ao-smooth is always guided by depth)")
        from .scene import bilateral_params, spatial_box, range_step
        cutoff = 16 if args.smooth_range is None else args.smooth_range
        scale = 8.0 if args.smooth_depth_scale is None else args.smooth_depth_scale
        try:
            for name, r, guide in (("--smooth", args.smooth, args.smooth_guide or "colour"), ("--ao-smooth", args.ao_smooth, "depth")):
                if r is None:
                    continue
                if not 1 <= r <= 7:
                    raise ValueError(name + " takes a radius 1..7")
                if not 0 <= cutoff <= 255:
                    raise ValueError("--smooth-range takes 0..255")
                p = bilateral_params(spatial_box(2 * r + 1, 2 * r + 1), range_step(cutoff), guide=guide, depth_scale=scale, edge="clamp")
                if name == "--smooth":
                    args.smooths.append(p)
                else:
                    args.ao_smooth_params = p
        except ValueError as e:
            ap.error(str(e))
    args.resize = None
    if args.out_size is not None:
        try:
            w, h = (int(v) for v in args.out_size.lower().split("x"))
        except ValueError:
            ap.error("--out-size takes two integers: WxH")
        if args.ssaa > 1:
            ap.error("--out-size does not go with --ssaa: render large (-W, -H) and resize with --resize-filter area instead")
        if args.gpus > 1 or args.view != "frame":
            ap.error("--out-size resizes the colour frame of one GPU: use --gpus 1 and --view frame")
        from .scene import resize_params
        try:
            resize_params(args.width, args.height, w, h, args.resize_filter, "--out-size")
        except ValueError as e:
            ap.error(str(e))
        args.resize = (w, h, args.resize_filter)
    args.y4m = bool(args.out) and args.out.lower().endswith(".y4m")
    if args.y4m:
        if args.gpus > 1 or args.view != "frame" or args.seconds > 0:
            ap.error("--out NAME.y4m converts the colour frames of one GPU, by frame count: use --gpus 1, --frames and --view frame")
        if args.shutter or args.shared_shadows:
            ap.error("--out NAME.y4m writes every frame of the run: not with --shutter (one average of the run's last frames) or --shared-shadows (one frame)")
        if args.fps < 1:
            ap.error("--fps must be >= 1")
    if args.gpus < 1:
        ap.error("--gpus must be >= 1")
    if args.instances < 1:
        ap.error("--instances must be >= 1")

    # --gpus N > 1 outside a launcher: start the N ranks from here, before anything touches a GPU
    world_env = os.environ.get("WORLD_SIZE")
    if args.gpus > 1 and world_env is None:
        from .sharded import launch_ranks
        return launch_ranks(args.gpus, "tiny_renderer_amd.cli", list(argv) if argv is not None else sys.argv[1:])
    world = int(world_env or "1")
    if world != args.gpus:
        raise SystemExit("--gpus %d does not match WORLD_SIZE %d" % (args.gpus, world))
    sharded = world > 1 or os.environ.get("TR_CLI_FORCE_DIST") == "1"
    rank = int(os.environ.get("RANK", "0"))
    say = print if rank == 0 else (lambda *a, **k: None)

    import tiny_renderer_amd as T

    if args.synthetic:
        mesh, texs = T.synthetic_scene()
    else:
        say("loading model from: %s/model.obj" % args.asset_path)
        mesh, texs = T.load_assets(args.asset_path)
    args.mesh, args.texs = mesh, texs
    say("number of vertices in a model: %d" % mesh["pos"].shape[0])
    say("number of polygons in a model: %d" % mesh["idx"].shape[0])
    say("cooking up a scene with '%s' shader pipeline" % args.pipeline)
    if sharded:
        import torch
        import torch.distributed as dist
        from .sharded import ShardedScene
        if os.environ.get("TR_CLI_IMPORT_CHECK") == "1":   # test hook: a rank started the way launch_ranks starts it
            print("rank %d of %d: imports ok" % (rank, world))
            return 0
        if args.seconds > 0:
            # every rank must render the same frames: wall-clock driven angles would differ per process
            raise SystemExit("--seconds (the time-based loop) runs on one GPU: use --frames with --gpus")
        if args.view != "frame":
            raise SystemExit("--view %s needs the whole z / shadow buffer on one GPU: use --gpus 1" % args.view)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29513")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        local = int(os.environ.get("LOCAL_RANK", "0"))
        n_dev = torch.cuda.device_count()
        if world > n_dev and not args.exchange.startswith("peer"):
            raise SystemExit("%d ranks on %d GPU(s): RCCL needs a device per rank -- use --exchange peer to run several ranks "
                             "on one GPU" % (world, n_dev))
        local %= max(n_dev, 1)
        torch.cuda.set_device(local)
        if args.exchange == "torch":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group("gloo")   # (the library's exchanges only need a rendezvous for their records)
        if dist.get_world_size() != args.gpus:
            raise SystemExit("process group has %d ranks, --gpus says %d" % (dist.get_world_size(), args.gpus))
        scene = ShardedScene(args.width, args.height, mesh, texs, args.pipeline, device=local, exchange=args.exchange)
    else:
        if args.ssaa > 1:
            say("supersampling: rendering %d x %d" % (args.width * args.ssaa, args.height * args.ssaa))
        # (--shutter N: the last N frames of the call must still exist when it ends -- a launch of N frames, N slots)
        scene = T.Scene(args.width * args.ssaa, args.height * args.ssaa, mesh, texs, args.pipeline, device=args.device,
                        frames_per_launch=args.shutter)
    if args.instance_yaw is not None:
        say("instances: %d x %d grid, cell (i, j) turned by (i * %d + j) * %g degrees about y"
            % (args.instances, args.instances, args.instances, args.instance_yaw))
        scene.set_instance_transforms(yawed_grid(T, args.instances, args.instance_yaw))
    elif args.instances > 1:
        say("instances: %d x %d grid" % (args.instances, args.instances))
        scene.set_instances(T.grid_instances(args.instances))
    if args.morph_to:
        say("morph target: %s, weight %g" % (args.morph_to, args.morph_weight))
        scene.set_morph_targets(*T.morph_deltas(mesh, T.load_obj(args.morph_to)))
        scene.set_morph_weights([args.morph_weight])
    if args.bend is not None:
        say("two-bone rig: upper bone turned about z by %g degrees" % args.bend)
        scene.set_skin(*bend_rig(mesh), n_bones=2)
        scene.set_bone_palette(bend_palette(T, args.bend))
    if args.paint_path:
        if sharded:
            raise SystemExit("--paint-with needs one scene of the whole frame (--gpus 1)")
        th, tw = texs[0].shape[:2]
        say("diffuse texture painted with: %s/model.obj ('%s' shader pipeline, %d x %d)"
            % (args.paint_path, args.paint_shader or args.pipeline, tw, th))
        mesh3, texs3 = T.load_assets(args.paint_path)
        painter = T.Scene(tw, th, mesh3, texs3, args.paint_shader or args.pipeline, device=args.device)
        painter.clear()
        painter.set_light_direction([float(np.sin(args.light_angle)), 0.0, float(np.cos(args.light_angle))])
        painter.set_camera([float(np.sin(args.camera_angle)), 0.0, float(np.cos(args.camera_angle))], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0])
        painter.render()
        scene.set_texture_from(painter, 0)
        scene.sync()       # (the texture is in place: the painter can go)
        painter.close()
    args.with_scene = None
    if args.with_path:
        say("second model from: %s/model.obj ('%s' shader pipeline, at %s)" % (args.with_path, args.with_shader or args.pipeline,
                                                                              args.with_offset))
        mesh2, texs2 = T.load_assets(args.with_path)
        # (both scenes store their depth: the merge reads it -- include/tiny_renderer.h, tr_scene_composite)
        args.with_scene = T.Scene(scene.width, scene.height, mesh2, texs2, args.with_shader or args.pipeline, device=args.device,
                                  store_depth=True, instances=np.array([args.with_offset + [1.0]], np.float32))
    rc = _run(args, T, scene, sharded, rank, say)
    if sharded:
        import torch.distributed as dist
        scene.close()   # (collective: nobody unmaps a slot a peer may still be reading)
        dist.barrier()
        dist.destroy_process_group()
    return rc


def yawed_grid(T, n, degrees):
    """--instance-yaw: grid_instances(n)'s offsets and scale as a transform table, cell k = i * n + j turned by
    k * degrees about y."""
    grid = T.grid_instances(n)
    yaw = np.deg2rad(np.arange(n * n, dtype=np.float64) * degrees)
    return T.rotation_instances(yaw, 0.0, 0.0, grid[:, 0:3], grid[:, 3])


def morph_wave(n_frames, weight):
    """--morph-to over --frames N: [N, 1] weights, a triangle wave from 0 up to `weight` and back, one period per call."""
    t = np.arange(n_frames, dtype=np.float64) / max(n_frames, 1)
    return (weight * (1.0 - np.abs(2.0 * t - 1.0))).astype(np.float32).reshape(n_frames, 1)


def bend_rig(mesh):
    """--bend: (bones [n_pos, 4] uint32, weights [n_pos, 4] float32) of a two-bone rig -- bone 0 holds the lower part of
    the model, bone 1 the upper, blended by a smooth step in height over the middle third (the weights sum to one)."""
    y = np.asarray(mesh["pos"], np.float64).reshape(-1, 3)[:, 1]
    lo, hi = float(y.min()), float(y.max())
    t = np.clip(((y - lo) / max(hi - lo, 1e-30) - 1.0 / 3.0) * 3.0, 0.0, 1.0)
    upper = t * t * (3.0 - 2.0 * t)
    bones = np.zeros((y.shape[0], 4), np.uint32)
    bones[:, 1] = 1
    weights = np.zeros((y.shape[0], 4), np.float32)
    weights[:, 1] = upper.astype(np.float32)
    weights[:, 0] = np.float32(1.0) - weights[:, 1]
    return bones, weights


def bend_palette(T, degrees):
    """--bend: [2, 24] -- bone 0 at rest, bone 1 turned about z by `degrees` (`degrees` an array [N]: [N, 2, 24], one
    palette per frame)."""
    d = np.atleast_1d(np.asarray(degrees, np.float64))
    pal = np.stack([T.rotation_instances([0.0, 0.0], 0.0, [0.0, np.deg2rad(a)], np.zeros((2, 3)), 1.0) for a in d])
    return pal if np.ndim(degrees) else pal[0]


def _run(args, T, scene, sharded, rank, say):

    if args.seconds > 0:
        # app.rs:12-13,160-165,173-199,230-246: angles advance by speed * frame time; a frame counter is
        # printed and reset whenever more than a second has passed
        camera_speed = 3.0
        ca, la = np.float32(args.camera_angle), np.float32(args.light_angle)
        start = last = fps_t = time.perf_counter()
        fps_counter, img = 0, None
        while True:
            now = time.perf_counter()
            if now - start >= args.seconds:
                break
            ca = np.float32(ca + camera_speed * (now - last))
            last = now
            scene.clear()
            scene.set_light_direction([float(np.sin(la)), 0.0, float(np.cos(la))])
            scene.set_camera([float(np.sin(ca)), 0.0, float(np.cos(ca))], [0, 0, 0], [0, 1, 0])
            scene.render()
            if not args.no_readback:
                img = _view(scene, args.view, args.ssaa, args.resize)
            elif fps_counter % 64 == 63:
                scene.sync()  # keep the queue bounded
            fps_counter += 1
            if now - fps_t > 1.0:
                say("FPS --- %d" % fps_counter)
                fps_counter, fps_t = 0, now
        scene.sync()
        if args.out:
            img = _view(scene, args.view, args.ssaa, args.resize)
            if rank == 0:
                write_frame(T, args.out, img)
        return 0

    t0 = time.perf_counter()
    angles = [np.float32(args.camera_angle + (2.0 * np.pi * f / args.frames if args.frames > 1 else 0.0))
              for f in range(args.frames)]
    la = np.float32(args.light_angle)
    if args.y4m:
        return _run_y4m(args, T, scene, angles, la, say, t0)
    if args.frames > 1 or args.shutter:
        # many frames: the library's throughput path (the same frames, several per kernel launch; with --gpus every
        # rank renders its band of a group, and the bands are exchanged frame by frame)
        p = np.zeros((args.frames, 12), np.float32)
        p[:, 0:3] = [float(np.sin(la)), 0.0, float(np.cos(la))]
        for f, ca in enumerate(angles):
            p[f, 3:6], p[f, 6:9], p[f, 9:12] = [float(np.sin(ca)), 0.0, float(np.cos(ca))], [0, 0, 0], [0, 1, 0]
        if args.morph_to:
            scene.render_frames(p, morph_weights=morph_wave(args.frames, args.morph_weight))
        elif args.bend is not None:
            scene.render_frames(p, bone_palettes=bend_palette(T, args.bend * np.arange(1, args.frames + 1) / args.frames))
        else:
            scene.render_frames(p)
        angles = []
    if args.shared_shadows:
        # one frame, pass by pass: both light-space passes, the shadow buffers merged both ways (each scene then holds
        # the buffer of both models), both colour passes; the composite below finishes the picture
        other = args.with_scene
        for s in (scene, other):
            s.clear()
            s.set_light_direction([float(np.sin(la)), 0.0, float(np.cos(la))])
            s.set_camera([float(np.sin(angles[0])), 0.0, float(np.cos(angles[0]))], [0, 0, 0], [0, 1, 0])
        scene.render_shadow_pass(), other.render_shadow_pass()
        scene.shadow_merge(other), other.shadow_merge(scene)
        scene.render_colour_pass(), other.render_colour_pass()
        scene.composite(other)
        angles = []
    for ca in angles:
        scene.clear()                                                        # app.rs:170
        scene.set_light_direction([float(np.sin(la)), 0.0, float(np.cos(la))])   # app.rs:203-208
        scene.set_camera([float(np.sin(ca)), 0.0, float(np.cos(ca))], [0, 0, 0], [0, 1, 0])  # app.rs:200-209
        scene.render()                                                       # app.rs:210
    if args.with_scene is not None and not args.shared_shadows:
        # the second model under the last frame's camera and light, merged into the picture before it is read
        ca = np.float32(args.camera_angle + (2.0 * np.pi * (args.frames - 1) / args.frames if args.frames > 1 else 0.0))
        other = args.with_scene
        other.clear()
        other.set_light_direction([float(np.sin(la)), 0.0, float(np.cos(la))])
        other.set_camera([float(np.sin(ca)), 0.0, float(np.cos(ca))], [0, 0, 0], [0, 1, 0])
        other.render()
        scene.composite(other)
    if args.shutter:
        scene.accumulate_in_place(args.shutter)
    _post(args, T, scene, say)
    img = _view(scene, args.view, args.ssaa, args.resize)
    dt = time.perf_counter() - t0
    say("FPS --- %d" % int(args.frames / dt if dt > 0 else 0))              # app.rs:238
    if args.out and rank == 0:
        write_frame(T, args.out, img)
    return 0


def _post(args, T, scene, say):
    """The stage options on the scene's current frame, in their order (after --with and --shutter)."""
    if args.ao:
        scene.ambient_occlusion(radius=args.ao, rings=args.ao_rings, grey=args.ao_grey)
        if args.ao_smooth_params is not None:   # in place, directly behind the occlusion: the depth it was taken from guides the blur
            scene.bilateral(args.ao_smooth_params)
    if args.backdrop_spec is not None:
        # in place, where nothing is drawn: depth of field, bloom and everything later see the backdrop
        spec = args.backdrop_spec
        back = _pinned_layer(scene, "backdrop", lambda: T.load_tga(spec) if isinstance(spec, str) else T.layer_gradient(scene.width, scene.height, spec[0], spec[1]))
        scene.layer(back, where="undrawn")
    if args.projector_view is not None:
        _projector(args, T, scene, say)
    if args.relight is not None:
        _relight(args, T, scene, say)
    if args.fog_colour is not None or args.depth_view is not None or args.depth_contours is not None:
        # in place, under the blur and the bloom; a frame with nothing drawn has no span and only its background to fog
        try:
            z0, scale = T.ramp_span_auto(scene, 256) if args.fog_span == "auto" else T.ramp_span(args.fog_span[0], args.fog_span[1], 256)
        except ValueError as e:
            say("depth ramp --- %s: the span is 1,0" % e)
            z0, scale = T.ramp_span(1.0, 0.0, 256)
        if args.depth_view is not None:
            scene.set_ramp(T.ramp_grey(256)[::-1].copy() if args.depth_view == "grey" else T.ramp_false_colour(256))
            scene.ramp(z0, scale)
        if args.depth_contours is not None:
            scene.set_ramp(T.ramp_contours(256, 256 // args.depth_contours))
            scene.ramp(z0, scale)
        if args.fog_colour is not None:
            scene.set_ramp(T.ramp_fog(args.fog_colour, 256, args.fog_kind, args.fog_density))
            scene.ramp(z0, scale, undrawn=args.fog_colour + ((255,) if args.fog_background else (0,)))
    if args.dof_autofocus:
        # the median depth of what is drawn in the central quarter; a picture with nothing there stays sharp
        w, h = scene.width, scene.height
        focus = T.depth_median(scene, (w // 4, h // 4, max(1, w // 2), max(1, h // 2)))
        if focus is None:
            say("autofocus --- nothing drawn in the central quarter: no depth of field")
        else:
            say("autofocus --- z %r" % focus)
            args.dof = T.dof_params(focus, args.dof_scale, max_radius=args.dof_radius, background_radius=args.dof_background,
                                    flags=1 if args.dof_show_coc else 0, range=args.dof_range)
    if args.dof is not None:
        scene.depth_of_field(args.dof)
    if args.bloom_params is not None:
        scene.bloom(args.bloom_params)
    if args.levels is not None:
        args.grade_lut = T.lut_auto_levels(scene.get_frame_stats(), args.levels[0], args.levels[1])
    if args.grade_lut is not None:
        scene.set_lut(args.grade_lut)
        scene.grade()
    if args.outline_params is not None:
        scene.outline(args.outline_params)
    if args.wire_colour is not None:
        # in place, after the outlines and before the filter, which smooths the lines; --wire-only clears first: the lines
        # then stand alone on black and no depth is read
        scene.set_lines(T.wireframe_lines(scene, args.mesh, args.wire_colour))
        if args.wire_only:
            scene.clear()
        scene.lines(args.wire_width, depth_test=not (args.wire_xray or args.wire_only), depth_bias=args.wire_bias)
    # in place, after the lines and before the filter: each keeps the seeds (the model), so only its surroundings -- or,
    # under --inner-glow, its inside near the border -- change
    if args.inner_glow_colour is not None:
        table, step = T.ramp_glow(args.inner_glow_colour, args.glow_radius)
        scene.set_ramp(table)
        scene.distance_ramp(args.glow_radius, step, invert=True, mode="add", keep_seeds=True)
    if args.glow_colour is not None:
        table, step = T.ramp_glow(args.glow_colour, args.glow_radius)
        scene.set_ramp(table)
        scene.distance_ramp(args.glow_radius, step, mode="add", keep_seeds=True)
    if args.stroke_colour is not None:
        table, step = T.ramp_stroke(args.stroke_colour, args.stroke_width)
        scene.set_ramp(table)
        scene.distance_ramp(args.stroke_width + 1, step, keep_seeds=True)
    if args.aa_params is not None:
        scene.antialias(args.aa_params)
    for grid, wp in args.warps:   # in place: --stats, --ssaa and --out-size see the warped frame
        scene.set_warp(grid, args.width, args.height)
        scene.warp(wp)
    for cp in args.convolves:     # in place, after the warps: --stats, --ssaa and --out-size see the filtered frame
        scene.convolve(cp)
    for rp in args.ranks:         # in place, after the convolves: erode, dilate, median, despeckle
        scene.rank(rp)
    for bp in args.smooths:       # in place, after the ranks: edge-preserving smoothing
        scene.bilateral(bp)
    if args.overlay is not None:   # in place, after the convolves: --stats, --ssaa, --out-size and y4m output see the layered frame
        scene.layer(_pinned_layer(scene, "overlay", lambda: T.load_tga(args.overlay)), args.overlay_at[0], args.overlay_at[1], args.overlay_mode,
                    args.overlay_opacity)
    if args.vignette is not None:
        scene.layer(_pinned_layer(scene, "vignette", lambda: T.layer_vignette(scene.width, scene.height, args.vignette)), mode="multiply")
    if args.stats:
        st = scene.get_frame_stats(depth=True)
        say("stats --- pixels %d drawn %d nan %d z [%r, %r] box %r luma 1%% %d 50%% %d 99%% %d"
            % (st.n_pixels, st.n_drawn, st.n_nan, float(st.z_min), float(st.z_max), st.box,
               T.hist_percentile(st.luma, 0.01), T.hist_percentile(st.luma, 0.5), T.hist_percentile(st.luma, 0.99)))


def _parse_lights(args):
    """The --light options as plain values: {"lights": [(kind, groups of floats)], "ambient", "specular"}.  ValueError in
    the option's words for a malformed one; the values themselves are checked by the builders when the lights are made."""
    def groups(text, option, shape_min, shape_max):
        parts = [[float(v) for v in g.split(",")] for g in text.split(":")]
        sizes = [len(g) for g in parts]
        if not (len(shape_min) <= len(parts) <= len(shape_max)) or sizes != list(shape_max[:len(parts)]):
            raise ValueError("%s takes %s" % (option, {"--light-point": "X,Y,Z:R,G,B[:INTENSITY[:FALLOFF]]", "--light-dir": "X,Y,Z:R,G,B[:INTENSITY]",
                                                       "--light-spot": "X,Y,Z:AX,AY,AZ:R,G,B:INNER,OUTER[:INTENSITY[:FALLOFF]]"}[option]))
        return parts
    lights = []
    for t in args.light_point:
        lights.append(("point", groups(t, "--light-point", (3, 3), (3, 3, 1, 1))))
    for t in args.light_spot:
        lights.append(("spot", groups(t, "--light-spot", (3, 3, 3, 2), (3, 3, 3, 2, 1, 1))))
    for t in args.light_dir:
        lights.append(("directional", groups(t, "--light-dir", (3, 3), (3, 3, 1))))
    if len(lights) > 8:
        raise ValueError("at most 8 lights in all")
    ambient = [0, 0, 0] if args.light_ambient is None else [int(v) for v in args.light_ambient.split(",")]
    if len(ambient) != 3 or min(ambient) < 0 or max(ambient) > 255:
        raise ValueError("--light-ambient takes R,G,B, each 0..255")
    specular = (0.0, 0)
    if args.light_specular is not None:
        sk = args.light_specular.split(",")
        if len(sk) != 2 or not 0 <= int(sk[1]) <= 10 or not float(sk[0]) >= 0:
            raise ValueError("--light-specular takes S,K with S >= 0 and K 0..10")
        specular = (float(sk[0]), int(sk[1]))
    return {"lights": lights, "ambient": ambient, "specular": specular}


def _relight(args, T, scene, say):
    """The --light options: the lights laid on the current frame in place, over the projector's image and under fog and
    everything later.  The matrix is the i_vpmv of the frame's camera; its eye stands 5 units behind look_from."""
    cam = getattr(scene, "_camera", None)
    if cam is None:   # (frames rendered as a group: the last one's camera)
        ca = np.float32(args.camera_angle + (2.0 * np.pi * (args.frames - 1) / args.frames if args.frames > 1 else 0.0))
        cam = ([float(np.sin(ca)), 0.0, float(np.cos(ca))], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0])
    st, view = T.prepare_uniforms(2, scene.width, scene.height, getattr(scene, "_light", (0.0, 0.0, 1.0)), *cam)
    if st != 0:
        raise SystemExit("--light-*: the camera's matrix is singular")
    eye = [float(cam[0][i]) + 5.0 * float(view.camera_direction[i]) for i in range(3)]
    spec, shin = args.relight["specular"]
    lights = []
    try:
        for kind, g in args.relight["lights"]:
            if kind == "point":
                lights.append(T.light_point(g[0], g[1], g[2][0] if len(g) > 2 else 1.0, g[3][0] if len(g) > 3 else 0.0, spec, shin))
            elif kind == "spot":
                lights.append(T.light_spot(g[0], g[1], g[3][0], g[3][1], g[2], g[4][0] if len(g) > 4 else 1.0, g[5][0] if len(g) > 5 else 0.0, spec, shin))
            else:
                lights.append(T.light_directional(g[0], g[1], g[2][0] if len(g) > 2 else 1.0, spec, shin))
        albedo = None if args.light_albedo is None else args.light_albedo == "on"
        p = T.relight_params(view, eye, args.relight["ambient"], args.light_mode, 256, albedo, args.show_normals)
    except ValueError as e:
        raise SystemExit("--light-*: %s" % e)
    say("relight --- %d light%s, %s%s" % (len(lights), "" if len(lights) == 1 else "s", args.light_mode, ", normals" if args.show_normals else ""))
    scene.relight(p, lights)


def _projector(args, T, scene, say):
    """--projector: the image cast onto the current frame in place from the projector's camera, under fog and everything
    later.  With --projector-shadows a second scene of the same mesh and of the image's size is rendered from that camera
    (it stores its depth) and passed as the occluder; it is made once and kept with the scene."""
    image = _pinned_layer(scene, "projector", lambda: T.load_tga(args.projector))
    ph, pw = image.shape[:2]
    cam = getattr(scene, "_camera", None)
    if cam is None:   # (frames rendered as a group: the last one's camera)
        ca = np.float32(args.camera_angle + (2.0 * np.pi * (args.frames - 1) / args.frames if args.frames > 1 else 0.0))
        cam = ([float(np.sin(ca)), 0.0, float(np.cos(ca))], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0])
    light = getattr(scene, "_light", (0.0, 0.0, 1.0))
    stand, at, up = args.projector_view[0], args.projector_view[1], list(cam[2])
    st, view = T.prepare_uniforms(2, scene.width, scene.height, light, *cam)
    st2, proj = T.prepare_uniforms(0, pw, ph, light, stand, at, up)
    if st != 0 or st2 != 0:
        raise SystemExit("--projector: a camera's matrix is singular")
    occluder = None
    if args.projector_shadows:
        occluder = scene.__dict__.get("_cli_projector_scene")
        if occluder is None:
            occluder = scene.__dict__["_cli_projector_scene"] = T.Scene(pw, ph, args.mesh, args.texs, "default", device=args.device, store_depth=True)
        occluder.clear()
        occluder.set_light_direction(list(light)), occluder.set_camera(stand, at, up)
        occluder.render()
    say("projector --- %s (%d x %d) from %s at %s%s" % (args.projector, pw, ph, stand, at, ", shadowed" if occluder is not None else ""))
    scene.projector(T.projector_matrix(view, proj), image, occluder, mode=args.projector_mode, opacity=args.projector_opacity,
                    soft=args.projector_soft, depth_bias=args.projector_bias if occluder is not None else 0.0)


def _pinned_layer(scene, name, make):
    """The layer `name` -- make() gives it, [h, w, 3 | 4] uint8 -- in a page-locked array of the scene's, which k_layer reads
    through its mapped address; made once and kept with the scene: a y4m run blends the same layers into every frame."""
    cache = scene.__dict__.setdefault("_cli_layers", {})
    if name not in cache:
        image = make()
        cache[name] = scene.pinned_layer(image.shape[1], image.shape[0], image.shape[2])
        cache[name][...] = image
    return cache[name]


def _run_y4m(args, T, scene, angles, la, say, t0):
    """--out NAME.y4m: every frame of the run rendered, sent through the stage options and converted on the GPU into one
    of TWO page-locked blocks, so that frame f + 1 is rendered and converted while frame f is written to the file.  With
    --out-size or --ssaa the resized or resolved image stays on the device and is converted from there."""
    light = [float(np.sin(la)), 0.0, float(np.cos(la))]
    w, h = scene.width, scene.height
    small = None
    if args.resize is not None or args.ssaa > 1:
        import torch
        w, h = (args.resize[0], args.resize[1]) if args.resize is not None else (scene.width // args.ssaa, scene.height // args.ssaa)
        small = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")
    blocks = [scene.pinned_yuv(args.yuv_layout, w, h) for _ in range(2)]
    yuv = dict(layout=args.yuv_layout, matrix=args.yuv_matrix, range=args.yuv_range)
    weights = morph_wave(args.frames, args.morph_weight) if args.morph_to else None
    bends = bend_palette(T, args.bend * np.arange(1, args.frames + 1) / args.frames) if args.bend is not None else None
    with T.Y4MWriter(args.out, w, h, args.fps, args.yuv_layout, args.yuv_range) as out:
        for f, ca in enumerate(angles):
            p = np.zeros((1, 12), np.float32)
            p[0, 0:3], p[0, 3:6], p[0, 6:9], p[0, 9:12] = light, [float(np.sin(ca)), 0.0, float(np.cos(ca))], [0, 0, 0], [0, 1, 0]
            if weights is not None:
                scene.render_frames(p, morph_weights=weights[f:f + 1])
            elif bends is not None:
                scene.render_frames(p, bone_palettes=bends[f:f + 1])
            else:
                scene.render_frames(p)
            if args.with_scene is not None:
                other = args.with_scene
                other.clear()
                other.set_light_direction(light)
                other.set_camera([float(np.sin(ca)), 0.0, float(np.cos(ca))], [0, 0, 0], [0, 1, 0])
                other.render()
                scene.composite(other)
            _post(args, T, scene, say)
            block = blocks[f % 2]
            if small is None:
                scene.to_yuv_into(block, **yuv)
            else:
                if args.resize is not None:
                    scene.resize_into(small, *args.resize)
                else:
                    scene.resolve_into(args.ssaa, small.data_ptr())
                scene.to_yuv_from(small, target=block, **yuv)
            scene.flush()
            if f > 0:   # (frame f is on its way: write frame f - 1, whose block the sync below has made whole)
                out.write(blocks[(f - 1) % 2])
            scene.sync()
        out.write(blocks[(len(angles) - 1) % 2])
    dt = time.perf_counter() - t0
    say("FPS --- %d" % int(args.frames / dt if dt > 0 else 0))
    print("wrote %s (%d frames)" % (args.out, len(angles)))
    return 0


def _view(scene, view, ssaa=1, resize=None):
    if resize is not None:   # (--view frame, --ssaa 1: main() has seen to it)
        return scene.resize(*resize)
    if view == "frame":
        return scene.resolve(ssaa) if ssaa > 1 else scene.get_frame_buffer()
    return {"z": scene.get_z_buffer, "shadow": scene.get_shadow_buffer}[view]()


def write_frame(T, path, img):
    if path.lower().endswith(".tga"):
        T.save_tga(path, img)
    elif path.lower().endswith(".png"):
        T.save_png(path, img)
    else:
        with open(path, "wb") as fh:
            fh.write(b"P6\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
            fh.write(img.tobytes())
    print("wrote %s" % path)


if __name__ == "__main__":
    sys.exit(main())
