/*
 * g4s_render_maps.h -- C ABI of the fused map post-processing that follows the rasterizer in
 * G4Splat's `render()`, libg4s_hip.so.
 *
 * Replaces the ~15 element-wise torch kernels of
 *   2d-gaussian-splatting/gaussian_renderer/__init__.py:117-164   (alpha / normal / depth maps)
 *   2d-gaussian-splatting/utils/point_utils.py:9-37               (depths_to_points, depth_to_normal)
 * by ONE forward and ONE backward kernel (plus a one-thread camera-algebra kernel).  The reference has
 * no C++ interface for this step (it is Python); the entry points below are what a maintainer would
 * call from `render()` through a `torch.autograd.Function` -- g4splat_amd/render_maps.py is that binding.
 *
 * Conventions as in g4s_rasterizer.h: device pointers, planar [C,H,W] float32 maps, the caller's
 * hipStream_t as void*, int status + g4s_last_error().
 */
#ifndef G4S_RENDER_MAPS_H_INCLUDED
#define G4S_RENDER_MAPS_H_INCLUDED

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of device scratch both calls need (the derived camera: rotation, ray matrix, origin). */
size_t g4s_render_maps_workspace(void);

/*
 * Forward.  gaussian_renderer/__init__.py:117-164 with `allmap` = the rasterizer's [7,H,W] output
 * (0 = sum w*depth, 1 = alpha, 2..4 = view-space normal, 5 = median depth, 6 = distortion):
 *
 *   rend_alpha      [1,H,W] = allmap[1]                                            (:118)
 *   rend_normal     [3,H,W] = allmap[2:5] rotated to world space                   (:121-123)
 *   rend_normal_cam [3,H,W] = allmap[2:5]                                          (:122)
 *   rend_depth      [1,H,W] = nan_to_num(allmap[0] / allmap[1], 0, 0)              (:130-131)
 *   rend_dist       [1,H,W] = allmap[6]                                            (:134)
 *   surf_depth      [1,H,W] = rend_depth (1 - depth_ratio) + depth_ratio nan_to_num(allmap[5], 0, 0)   (:139)
 *   surf_normal     [3,H,W] = normalize(cross(dP/drow, dP/dcol)) * alpha, P = back-projected surf_depth,
 *                             central differences, zero on the 1-pixel border   (:142-146, point_utils.py:26-37)
 *   surf_normal_cam [3,H,W] = surf_normal rotated to view space                    (:149)
 *
 * world_view_transform / full_proj_transform: the camera's 4x4 matrices exactly as the reference
 * stores them (row-major torch tensors, row-vector convention, scene/cameras.py:55-57).
 */
int g4s_render_maps_forward(int width, int height, const float* allmap, const float* world_view_transform,
                            const float* full_proj_transform, float depth_ratio, float* rend_alpha, float* rend_normal,
                            float* rend_normal_cam, float* rend_depth, float* rend_dist, float* surf_depth,
                            float* surf_normal, float* surf_normal_cam, char* workspace, size_t workspace_bytes,
                            void* stream);

/*
 * Backward: dL/dallmap [7,H,W] (every element written) from the gradients of the eight maps; any
 * dL_* pointer may be NULL (= zero).  surf_depth is the forward's output.  Alpha is detached inside
 * surf_normal exactly as in the reference (:146).  Gather form, no atomics: bit-reproducible.
 */
int g4s_render_maps_backward(int width, int height, const float* allmap, const float* surf_depth,
                             const float* world_view_transform, const float* full_proj_transform, float depth_ratio,
                             const float* dL_rend_alpha, const float* dL_rend_normal, const float* dL_rend_normal_cam,
                             const float* dL_rend_depth, const float* dL_rend_dist, const float* dL_surf_depth,
                             const float* dL_surf_normal, const float* dL_surf_normal_cam, float* dL_dallmap,
                             char* workspace, size_t workspace_bytes, void* stream);

/* =====================================================================================================================
 * TSDF fusion of rendered depth maps and marching-cubes mesh extraction (g4splat_amd/csrc/tsdf/tsdf.hip).
 *
 * The step after training in the reference (2d-gaussian-splatting/utils/mesh_utils.py:73-182, GaussianExtractor with
 * open3d's ScalableTSDFVolume; render.py:57-106).  Modelled on that volume as the reference configures it, but the
 * semantics below are this library's own, stated exactly (tests/tsdf_ref.py restates them in numpy); nothing here is
 * claimed bit-equal to open3d.  All arithmetic is float32, round-to-nearest-even, correctly rounded / and sqrt, no
 * fused multiply-add (the library builds with -ffp-contract=off), evaluated left to right as written.
 *
 * Camera.  intrinsic = {fx, fy, cx, cy} as mesh_utils.py:45-70 (to_cam_open3d) derives them from
 *   projection_matrix @ ndc2pix (a centred camera: cx = (W-1)/2).  extrinsic = 16 floats, row-major, world -> camera
 *   = world_view_transform.T; rows 0..2 are used (E).  The camera -> world matrix C of the allocation is the rigid
 *   inverse of E computed in double precision and rounded to float once: C = [E3^T | -(E3^T t)], each component of
 *   E3^T t summed left to right.  Host pointers, read during the call.
 * Inputs per view.  depth [H,W] float32: pixel valid iff 0 < d <= depth_trunc (and, with a mask [H,W], mask >= 0.5).
 *   rgb [3,H,W] float32: each value is clamped to [0,1] (NaN -> 0), multiplied by 255 and truncated to an integer
 *   0..255 -- the reference's uint8 cast of rgb*255, defined also outside [0,1].
 * Volume.  Blocks of 8^3 voxels, voxel size v; voxel (i,j,k) (global integer coordinates) has its centre at
 *   ((i,j,k) + 0.5) * v.  Block (bx,by,bz) holds voxels 8*(bx,by,bz) + (0..7)^3, stored x fastest (lane = x + 8y + 64z).
 *   Key of a block: ((bx + 2^20) << 42) | ((by + 2^20) << 21) | (bz + 2^20), 64-bit; the table of the volume is the
 *   ascending list of keys with the pool slot of each.  A voxel holds tsdf, weight, colour[3] (0..255) as float32.
 *   Pool layout: tsdf[slot*512 + lane], weight[slot*512 + lane], colour[(slot*512 + lane)*3 + c].
 * Allocation.  Per valid pixel (u,v) with depth d: rx = (u - cx) / fx, ry = (v - cy) / fy; for z in {d - sdf_trunc,
 *   d + sdf_trunc} the camera point (rx*z, ry*z, z) is mapped by C (w_r = ((C_r0 x + C_r1 y) + C_r2 z) + C_r3) and
 *   divided by the block size B = 8 * v, giving a and b.  A pixel with any |a_i| or |b_i| >= 1e6 (or NaN) allocates
 *   nothing.  Otherwise the cells floor(a) .. floor(b) are walked by a 3-D DDA: start at floor(a); while the cell is not
 *   floor(b), among the axes i whose cell differs from floor(b_i) take the smallest
 *   t_i = ((cell_i + (b_i > a_i ? 1 : 0)) - a_i) / (b_i - a_i)  (ties: the lowest axis) and step that axis towards
 *   floor(b_i).  Every visited block is allocated -- a superset of the blocks the segment meets (a corner crossing
 *   visits one extra neighbour).  The walk stops after g4s_tsdf_blocks_per_pixel() blocks, a bound that exact
 *   arithmetic never reaches.  New blocks get the slots n_blocks, n_blocks+1, ... in ascending key order; their voxels
 *   start at tsdf = weight = colour = 0; voxel data never moves.
 * Integration of one view, for every voxel of every block the view allocated or touched (the set from the walk):
 *   p = voxel centre; (x,y,z) = E p (rows as above); skip unless z > 0; u = floor((fx*x)/z + cx + 0.5),
 *   v = floor((fy*y)/z + cy + 0.5) (round half up), skip unless 0 <= u <= W-1, 0 <= v <= H-1 and pixel (u,v) valid;
 *   a = (u - cx)/fx, b = (v - cy)/fy, sdf = (d - z) * sqrt((1 + a*a) + b*b); skip unless sdf > -sdf_trunc;
 *   t = min(1, sdf/sdf_trunc); tsdf <- (tsdf*w + t)/(w + 1); colour_c <- (colour_c*w + q_c)/(w + 1); w <- w + 1.
 * Extraction.  A voxel is valid iff its block is allocated and weight > 0.  A cube (lower corner voxel g, corners
 *   g + {0,1}^3) is valid iff its eight corners are; its configuration has bit c set iff tsdf(corner c) < 0, corner
 *   c = x | y << 1 | z << 2.  Each cube edge is owned by its lower-corner voxel; an edge carries a vertex iff its two
 *   voxels are valid, their signs (tsdf < 0) differ, and a valid cube contains it.  Vertex: e = f0 / (f0 - f1) (f0 at
 *   the owner), position ((g + 0.5) along the other axes, (g_a + 0.5) + e along the edge's axis) * v, colour
 *   (c0 + e*(c1 - c0)) / 255 per channel.  Triangles come from g4splat_amd/csrc/tsdf/tsdf_mc_table.h (generated by
 *   tools/gen_mc_table.py: crossing polygons walked over the cube faces, ambiguous faces separate the negative corners,
 *   fan triangulation from a vertex whose diagonals cross the cube's interior) and face towards positive tsdf, i.e.
 *   towards the cameras.  Comparisons and the division are IEEE float32 without flush-to-zero: a subnormal tsdf counts
 *   as its sign (-1e-40 is negative; +1e-40, 0.0 and -0.0 are not) and f0 / (f0 - f1) of subnormals is the correctly
 *   rounded quotient.  The library is built with the compiler's default denormal mode, which keeps them.
 * Order.  Vertices: blocks in ascending key, voxels x fastest, edges +x, +y, +z.  Triangles: blocks in ascending key,
 *   cubes (by lower corner) x fastest, the table's order.  No atomics anywhere: two runs are bit-identical.
 *
 * Sequence per view:  alloc_count (emits, sorts and uniques the keys, looks them up; reads back two counts) ->
 * the caller makes room (pool_blocks >= n_blocks + n_new, table arrays of n_blocks + n_new) -> merge (writes the new
 * table to keys_out / slots_out, which must not alias the old one) -> integrate.  The three calls share the workspace,
 * and merge / integrate use what alloc_count left in it.  Extraction: extract_count (reads back vertex and triangle
 * counts) -> extract_emit.  Keys are `long long` holding the unsigned packed value (bit 63 is always 0).
 * Every argument is checked on the host before anything is launched; capacities are the caller's: no kernel grows or
 * overflows anything.
 */

/* Key slots per pixel the allocation needs for this camera (>= 1), or a negative G4S_ERR_* for bad arguments. */
int g4s_tsdf_blocks_per_pixel(int width, int height, const float* intrinsic, float voxel_size, float sdf_trunc);

/* Bytes of device workspace for views of width x height with `blocks_per_pixel` key slots (width = 0: none) and for
 * the extraction of a volume of n_blocks blocks: the larger of the two. */
size_t g4s_tsdf_workspace(int width, int height, int blocks_per_pixel, int n_blocks);

/* counts[0] = blocks the view touches, counts[1] = of those, blocks not yet in the table (host int[2]). */
int g4s_tsdf_alloc_count(int width, int height, const float* depth, const float* mask, const float* intrinsic,
                         const float* extrinsic, float voxel_size, float sdf_trunc, float depth_trunc, int blocks_per_pixel,
                         const long long* keys, int n_blocks, int* counts, char* workspace, size_t workspace_bytes,
                         void* stream);

int g4s_tsdf_merge(int width, int height, int blocks_per_pixel, const long long* keys_in, const int* slots_in, int n_blocks,
                   int n_touched, int n_new, long long* keys_out, int* slots_out, float* tsdf, float* weight, float* color,
                   int pool_blocks, char* workspace, size_t workspace_bytes, void* stream);

int g4s_tsdf_integrate(int width, int height, const float* depth, const float* mask, const float* rgb,
                       const float* intrinsic, const float* extrinsic, float voxel_size, float sdf_trunc, float depth_trunc,
                       int blocks_per_pixel, int n_touched, float* tsdf, float* weight, float* color, int pool_blocks,
                       char* workspace, size_t workspace_bytes, void* stream);

/* totals[0] = vertices, totals[1] = triangles of the mesh (host int[2]). */
int g4s_tsdf_extract_count(const long long* keys, const int* slots, int n_blocks, const float* tsdf, const float* weight,
                           int pool_blocks, int* totals, char* workspace, size_t workspace_bytes, void* stream);

/* vertices [n_vertices,3], vertex_colors [n_vertices,3] (0..1), triangles [n_triangles,3]: the totals of extract_count
 * on the same volume and workspace (nothing is written beyond them). */
int g4s_tsdf_extract_emit(const long long* keys, const int* slots, int n_blocks, const float* tsdf, const float* weight,
                          const float* color, int pool_blocks, float voxel_size, float* vertices, float* vertex_colors,
                          int* triangles, int n_vertices, int n_triangles, char* workspace, size_t workspace_bytes,
                          void* stream);

/* =====================================================================================================================
 * Unbounded TSDF and dense marching cubes (g4splat_amd/csrc/tsdf/unbounded.hip).
 *
 * The reference's mesh extraction for unbounded scenes (2d-gaussian-splatting/utils/mesh_utils.py:184-279
 * extract_mesh_unbounded, utils/mcube_utils.py; render.py --unbounded): a TSDF over a lattice of the contracted,
 * normalised space, every view fused into every lattice point, marching cubes over the lattice, the vertices mapped back
 * to the world.  As above, the semantics are this library's own, stated exactly (tests/unbounded_ref.py restates them in
 * numpy): float32, round-to-nearest-even, correctly rounded / and sqrt, no fused multiply-add, evaluated left to right
 * as written.  min / max are IEEE minNum / maxNum (a NaN operand yields the other one).
 *
 * Views.  V views, fused in stack order.  View v has full_proj_transform M (16 floats, row-major, used as
 *   row-vector @ M: M[r][c] = M[4r + c]), a depth map [H,W] and -- for colours -- an rgb map [3,H,W], float32 device
 *   pointers.  W and H may differ between views (sizes = {W0, H0, W1, H1, ...}).
 * Lattice.  n points per axis over [-R, R]^3 of the contracted, normalised space (R = half_extent):
 *   c(i) = -R + float(i) * h, h = (2 * R) / float(n - 1); storage x fastest, idx = i + n * (j + n * k).  2 <= n and
 *   n^3 < 2^31.  Stated difference: the reference demands n % 512 == 0 and evaluates overlapping 512^3 crops, each with
 *   its own linspace and spacing; here it is one lattice and any n.
 * Point in contracted mode (lattice points, explicit points with contracted != 0, marching-cubes vertices):
 *   m = sqrt((y0*y0 + y1*y1) + y2*y2); if m < 1, u = y; otherwise s = 1 / (2 - m) and u_c = s * (y_c / m).  World point
 *   p_c = u_c * radius + center_c.  Truncation T = 5 * voxel_size, and if m > 1, T = T * (1 / (2 - min(m, 1.9))).  The
 *   expressions are evaluated as written also for m >= 2 (lattice corners reach 1.9 * sqrt(3)), where they give a
 *   mirrored or non-finite point -- the reference's arithmetic does the same; every comparison with NaN is false, so a
 *   NaN point is seen by no view.
 * Point in world mode (explicit points with contracted == 0; the vertex colours): p is given, T = 5 * voxel_size;
 *   center and radius are not read.
 * State per point: tsdf = 1, w = 1, colour = 0 -- the reference's prior observation of +1, which also darkens a colour
 *   seen n times by n / (n + 1); both quirks are reproduced.
 * Per view, in order:  h_c = ((p0*M[0][c] + p1*M[1][c]) + p2*M[2][c]) + M[3][c] for c = 0, 1, 3; z = h_3, px = h_0 / z,
 *   py = h_1 / z; inside = px > -1 && px < 1 && py > -1 && py < 1 && z > 0.  If inside, a bilinear sample with
 *   align_corners: ix = ((px + 1) / 2) * float(W - 1), x0 = floor(ix), x1 = min(x0 + 1, W - 1), fx = ix - x0, the same
 *   in y with H; w00 = (1-fx)*(1-fy), w10 = fx*(1-fy), w01 = (1-fx)*fy, w11 = fx*fy (first index x);
 *   d = ((d00*w00 + d10*w10) + d01*w01) + d11*w11, each rgb channel s_c likewise.  sdf = d - z.  The view is skipped
 *   unless inside && sdf > -T.  t = min(1, max(-1, sdf / T)); tsdf <- (tsdf*w + t) / (w + 1);
 *   colour_c <- (colour_c*w + s_c) / (w + 1); w <- w + 1.
 * Dense marching cubes over a lattice of tsdf values (any device array of n^3 floats).  Every point is valid.  A cube has
 *   its lower corner at (i,j,k), i,j,k < n-1; configuration bit c is set iff tsdf(corner c) < 0, corners numbered as in
 *   the TSDF section.  An edge is owned by its lower point and carries a vertex iff the signs (tsdf < 0) of its two points
 *   differ (subnormals count as their sign, as in the TSDF section).  e = f0 / (f0 - f1) (f0 at the owner); contracted
 *   position: c(.) on the other two axes and c(g_a) + e * h along the edge's axis; then un-contracted and un-normalised as a point in contracted mode; then each world
 *   coordinate q becomes min(max(q, -max_range), max_range) (the reference's default is 32; it clamps world units, the
 *   reference's own quirk; a NaN coordinate becomes -max_range).  Triangles come from
 *   g4splat_amd/csrc/tsdf/tsdf_mc_table.h and face positive tsdf (the reference's skimage orientation is not modelled).
 *   Order: vertices by owner point in storage order (x fastest), edges +x, +y, +z; triangles by cube in storage order,
 *   the table's order.  No atomics: two runs are bit-identical.  Vertices are shared by construction, so the reference's
 *   merge_vertices(digits_vertex=6) has no counterpart.
 * Vertex colours: the world-mode evaluation at the clamped vertices, its colour as it stands -- not divided by 255 (the
 *   rgb maps are used as floats here, unlike the bounded path).
 *
 * center = 3 host floats; full_proj [V,16], sizes [V,2] and the arrays of V map pointers are HOST arrays, read during the
 * call (the library packs them into a table in the workspace).  Every argument is checked on the host before anything is
 * launched; capacities are the caller's.  Sequence: utsdf_grid -> dense_mc_count (reads back two totals) -> the caller
 * allocates -> dense_mc_emit (same n, tsdf and workspace, untouched in between) -> utsdf_sample (world mode, colours).
 */

/* Bytes of device workspace of g4s_utsdf_grid / g4s_utsdf_sample for a stack of n_views views. */
size_t g4s_utsdf_workspace(int n_views);

/* tsdf [n^3]: the fused lattice, written once.  n_views = 0: every value is exactly 1. */
int g4s_utsdf_grid(int n, float half_extent, const float* center, float radius, float voxel_size, int n_views,
                   const float* full_proj, const int* sizes, const float* const* depth, float* tsdf, char* workspace,
                   size_t workspace_bytes, void* stream);

/* The same evaluation at explicit points [n_points,3] (device), contracted != 0: contracted mode, else world mode.
 * tsdf [n_points] and colour [n_points,3] are optional (at least one); colour needs the rgb maps. */
int g4s_utsdf_sample(int n_points, const float* points, int contracted, const float* center, float radius,
                     float voxel_size, int n_views, const float* full_proj, const int* sizes, const float* const* depth,
                     const float* const* rgb, float* tsdf, float* colour, char* workspace, size_t workspace_bytes,
                     void* stream);

/* Bytes of device workspace of the dense marching cubes over n^3 points (0 for an n outside the lattice's range). */
size_t g4s_dense_mc_workspace(int n);

/* totals[0] = vertices, totals[1] = triangles (host int[2]; one host synchronisation). */
int g4s_dense_mc_count(int n, const float* tsdf, int* totals, char* workspace, size_t workspace_bytes, void* stream);

/* vertices [n_vertices,3] (world, clamped), triangles [n_triangles,3]: the totals of dense_mc_count (nothing is written
 * beyond them; with n_vertices = 0 nothing is written at all). */
int g4s_dense_mc_emit(int n, const float* tsdf, float half_extent, const float* center, float radius, float max_range,
                      float* vertices, int* triangles, int n_vertices, int n_triangles, char* workspace,
                      size_t workspace_bytes, void* stream);

/* =====================================================================================================================
 * Adaptive TSDF at points and marching tetrahedra (g4splat_amd/csrc/tsdf/tetra.hip).
 *
 * The reference's default mesh (scripts/extract_tetra_mesh.py -> 2d-gaussian-splatting/extract_mesh_adaptive_tsdf.py:259-377
 * marching_tetrahedra_with_binary_search; matcha/dm_extractors/adaptive_tsdf.py AdaptiveTSDF.integrate with the flags of
 * configs/adaptive_tetrahedralization/default.yaml; utils/tetmesh.py): a TSDF evaluated at the points of a tetrahedralisation,
 * marching tetrahedra over its cells, every crossing edge bisected against the same field.  As above, the semantics are
 * this library's own, stated exactly (tests/tetra_ref.py restates them in numpy): float32, round-to-nearest-even,
 * correctly rounded /, no fused multiply-add, evaluated left to right as written; min / max are IEEE minNum / maxNum.
 *
 * Views.  V views, fused in stack order.  View v has world_view_transform Wv and projection_matrix Pm (16 floats each,
 *   row-major, used as row-vector @ M: M[r][c] = M[4r + c]), a depth map [H,W] and -- for colours -- an rgb map [3,H,W],
 *   float32 device pointers.  W and H may differ between views (sizes = {W0, H0, W1, H1, ...}).
 * State per point p before the first view: tsdf = -1, w = 0, colour = 0.
 * Per view, in order:
 *   v_c = ((p0*Wv[0][c] + p1*Wv[1][c]) + p2*Wv[2][c]) + Wv[3][c] for c = 0, 1, 2;  z = v_2.
 *   q_c = ((v_0*Pm[0][c] + v_1*Pm[1][c]) + v_2*Pm[2][c]) + Pm[3][c] for c = 0, 1, 3;  qw = q_3 > znear ? q_3 : znear.
 *   ix = ((1 + q_0 / qw) * float(W)) / 2, iy = ((1 + q_1 / qw) * float(H)) / 2 -- W and H, not W - 1 and H - 1: the
 *   reference's pixel convention, kept.
 *   used = ix >= 0 && ix <= W-1 && iy >= 0 && iy <= H-1 && z > znear && z < zfar (every comparison with NaN is false).
 *   If used, a bilinear sample at (ix, iy) taken as pixel-index coordinates: x0 = floor(ix), x1 = min(x0 + 1, W - 1),
 *   fx = ix - x0, the same in y with H; w00 = (1-fx)*(1-fy), w10 = fx*(1-fy), w01 = (1-fx)*fy, w11 = fx*fy (first index x);
 *   d = ((d00*w00 + d10*w10) + d01*w01) + d11*w11, each rgb channel s_c likewise.  (The reference normalises (ix, iy) to
 *   [-1, 1] and grid_sample maps them back: a float32 round trip this contract does not make.)
 *   The view is skipped unless used && d > 0 && d - z >= -trunc_margin.
 *   dist = min((d - z) / trunc_margin, 1) -- no lower clamp --; tsdf <- (tsdf*w + dist) / (w + 1);
 *   colour_c <- min(max((colour_c*w + s_c) / (w + 1), 0), 1); w <- w + 1.
 *   A point no view accepts keeps tsdf = -1: unseen counts as inside, the reference's quirk.  Only this default flag set
 *   of AdaptiveTSDF.integrate exists (bilinear depth, obs_weight 1, every filter and weighting flag off).
 * Marching tetrahedra.  points are named by index < n_points < 2^31; tets [T,4] int32 (16-byte aligned), T < 2^29.  A point
 *   is occupied iff sdf > 0 (exactly 0, and NaN, are not).  Case bit c of a tet is set iff its corner c is occupied; a tet
 *   that names an index outside [0, n_points) is skipped (case 0) and none of its indices is used as an address.  A tet
 *   with one to three occupied corners has its crossing edges (exactly one end occupied) among the corner pairs
 *   (01, 02, 03, 12, 13, 23) = edge ids 0..5; an edge between points a, b has the key min(a,b) << 32 | max(a,b).
 *   Vertices: the distinct keys of all crossing edges in ascending key order; edges[i] = (lo, hi) of key i -- the
 *   reference's unique, occupied-on-one-end edges in torch.unique's order.  Triangles: tets in input order, each one's
 *   triangles in the order of g4splat_amd/csrc/tsdf/tsdf_mtet_table.h (tools/gen_mtet_table.py: one triangle for one or
 *   three occupied corners, a quad split along the crossings of opposite tet edges (02, 13), else (03, 12), for two; in a
 *   tet of positive orientation the normals point to the occupied corners -- the reference's table up to a rotation of each
 *   triple), each index the position of that edge's key among the vertices (binary search).  Stated difference: the
 *   reference emits all one-triangle tets before all two-triangle tets; here triangles stay in tet order.
 *   No atomics: two runs are bit-identical.
 * Bisection.  Per crossing edge (lo, hi): l = points[lo], r = points[hi], ls = sdf[lo].  `steps` times: m_c = (l_c + r_c) / 2;
 *   ms = the tsdf of the whole stack at m (as above, no colour); low = (ms < 0 && ls < 0) || (ms > 0 && ls > 0); if low,
 *   l <- m and ls <- ms; otherwise r <- m (so ms == 0 moves the right end).  vertices[i] = (l + r) / 2 per coordinate
 *   (steps = 0: the edge's midpoint).  An edge that names an index outside [0, n_points) gets three NaNs.
 *
 * world_view, projection [V,16], sizes [V,2] and the arrays of V map pointers are HOST arrays, read during the call (the
 * library packs them into a table in the workspace).  Every argument is checked on the host before anything is launched;
 * capacities are the caller's.  Sequence: atsdf_sample at the points -> mtet_count (reads back its totals) -> the caller
 * allocates -> mtet_emit (same tets, sdf and workspace, untouched in between) -> atsdf_bisect -> atsdf_sample (colours).
 */

/* Bytes of device workspace of g4s_atsdf_sample / g4s_atsdf_bisect for a stack of n_views views. */
size_t g4s_atsdf_workspace(int n_views);

/* The fused field at points [n_points,3] (device).  tsdf [n_points] and colour [n_points,3] are optional (at least one);
 * colour needs the rgb maps.  n_views = 0: every tsdf is exactly -1. */
int g4s_atsdf_sample(int n_points, const float* points, float trunc_margin, float znear, float zfar, int n_views,
                     const float* world_view, const float* projection, const int* sizes, const float* const* depth,
                     const float* const* rgb, float* tsdf, float* colour, char* workspace, size_t workspace_bytes,
                     void* stream);

/* vertices [n_edges,3]: every crossing edge (edges [n_edges,2], as g4s_mtet_emit writes them) bisected `steps` times
 * (0 .. 64) against the fused field; sdf [n_points] is that field at the points. */
int g4s_atsdf_bisect(int n_edges, const int* edges, int n_points, const float* points, const float* sdf, int steps,
                     float trunc_margin, float znear, float zfar, int n_views, const float* world_view,
                     const float* projection, const int* sizes, const float* const* depth, float* vertices,
                     char* workspace, size_t workspace_bytes, void* stream);

/* Bytes of device workspace of the marching tetrahedra over n_tets tets (0 for an n_tets outside 0 .. 2^29 - 1). */
size_t g4s_mtet_workspace(int n_tets);

/* totals[0] = vertices (crossing edges), totals[1] = triangles (host int[2]; two host synchronisations).  n_tets = 0 or
 * no crossing tet: both 0, nothing else is done. */
int g4s_mtet_count(int n_points, int n_tets, const int* tets, const float* sdf, int* totals, char* workspace,
                   size_t workspace_bytes, void* stream);

/* edges [n_edges,2], faces [n_faces,3]: the totals of mtet_count (nothing is written beyond them; with n_edges = 0
 * nothing is written at all). */
int g4s_mtet_emit(int n_points, int n_tets, const int* tets, const float* sdf, int* edges, int* faces, int n_edges,
                  int n_faces, char* workspace, size_t workspace_bytes, void* stream);

/* =====================================================================================================================
 * Mesh operations of the multi-resolution export (g4splat_amd/csrc/tsdf/mesh_ops.hip).
 *
 * What the reference does to its TSDF meshes before it evaluates them (2d-gaussian-splatting/render_multires.py:139-206,
 * utils/mesh_utils.py:22-43 post_process_mesh, utils/mesh_filter.py:6-32 filter_mesh), there through pytorch3d and
 * open3d on the host.  As with the TSDF, the semantics below are this library's own, stated exactly
 * (tests/mesh_ops_ref.py restates them in numpy).
 *
 * A mesh is vertices [V,3] float32, vertex_colors [V,3] float32, triangles [F,3] int32, all device pointers;
 * 3 * V and 3 * F are below 2^31.  Every output is a pure function of the input arrays -- independent of launch geometry
 * and scheduling -- and stable: surviving triangles and surviving vertices keep their relative order.  Only integer
 * atomics are used (compare-and-swap, min, add on 32- and 64-bit words).  Keep masks are unsigned char, 1 = keep.
 * No index is ever used unchecked: a triangle with an index outside [0, V) counts as having an unobserved vertex (A),
 * fails the edge-length test (D), and that index is written as -1 by a compaction (E).
 *
 * A. Observed vertices.  Cameras: world_view_transforms and full_proj_transforms [C,16], row-major 4x4 in the row-vector
 *   convention the cameras carry them in (point' = [p,1] @ M), device pointers.  For vertex p = (x,y,z) and matrix M:
 *   col_k(M) = ((x*M[0][k] + y*M[1][k]) + z*M[2][k]) + M[3][k] in float32, no contraction.  With P = full_proj and
 *   W = world_view of camera c: hx = col_0(P), hy = col_1(P), hw = col_3(P), w' = hw > 1e-6f ? hw : 1e-6f,
 *   inside = |hx / w'| < 1 and |hy / w'| < 1 (strict; one correctly rounded division each), zc = col_2(W),
 *   close = zc < near_trunc (no zc > 0 test: the reference has none).  observed(p) = inside and close for some camera.
 *   keep_unobserved: a triangle is kept unless all three of its vertices are observed.
 * B. Clusters.  Two triangles are adjacent iff they share an undirected edge {a,b}, a != b, by vertex index (not
 *   position); an edge used by three or more triangles joins all of them; a triangle with a repeated index still owns its
 *   other edges; sharing only a vertex does not connect.  labels[t] = the smallest triangle index in t's cluster (the
 *   transitive closure), sizes[t] = the number of triangles of that cluster.  Index values are only compared, never
 *   used as addresses.
 * C. keep_min_size: keep[t] = sizes[t] >= min_size.  keep_nondegenerate: keep[t] = the three indices are pairwise
 *   different.  (post_process_mesh = clusters, min_size = max(k-th largest cluster size, 50), compaction with vertices,
 *   keep_nondegenerate, compaction without vertices; g4splat_amd/mesh.py.)
 * D. keep_short_edges: per edge (a,b), (b,c), (c,a), in float64 from the float32 coordinates: d = p_a - p_b per axis,
 *   sqrt((dx*dx + dy*dy) + dz*dz) <= length_threshold; all three edges.
 * E. Compaction, two-phase.  compact_count: triangle t survives iff keep == NULL or keep[t] != 0; with compact_vertices,
 *   a vertex survives iff a surviving triangle names it; totals = {surviving vertices (n_vertices without
 *   compact_vertices), surviving triangles} (host int[2]; one host synchronisation).  compact_emit, same sizes,
 *   compact_vertices and workspace, the workspace untouched in between: the surviving triangles in order with their
 *   indices rewritten to the surviving vertices' new positions, and (with compact_vertices) the surviving vertices and
 *   colours in order; without compact_vertices only triangles_out is written.  Nothing is written beyond
 *   n_vertices_out / n_triangles_out.  Outputs must not alias inputs.
 * Every argument is checked on the host before anything is launched.
 */

/* observed [n_vertices]: 1 iff some camera sees the vertex inside its image and nearer than near_trunc. */
int g4s_mesh_observed_vertices(int n_vertices, const float* vertices, int n_cameras, const float* world_view_transforms,
                               const float* full_proj_transforms, float near_trunc, unsigned char* observed, void* stream);

int g4s_mesh_keep_unobserved(int n_triangles, const int* triangles, int n_vertices, const unsigned char* observed,
                             unsigned char* keep, void* stream);

int g4s_mesh_keep_min_size(int n_triangles, const int* sizes, int min_size, unsigned char* keep, void* stream);

int g4s_mesh_keep_nondegenerate(int n_triangles, const int* triangles, unsigned char* keep, void* stream);

int g4s_mesh_keep_short_edges(int n_triangles, const int* triangles, int n_vertices, const float* vertices,
                              double length_threshold, unsigned char* keep, void* stream);

/* Bytes of device workspace of g4s_mesh_cluster_triangles (edge table of at least 6 n_triangles slots, union-find). */
size_t g4s_mesh_cluster_workspace(int n_triangles);

/* labels, sizes [n_triangles] int32. */
int g4s_mesh_cluster_triangles(int n_triangles, const int* triangles, int* labels, int* sizes, char* workspace,
                               size_t workspace_bytes, void* stream);

size_t g4s_mesh_compact_workspace(int n_vertices, int n_triangles);

int g4s_mesh_compact_count(int n_vertices, int n_triangles, const int* triangles, const unsigned char* keep,
                           int compact_vertices, int* totals, char* workspace, size_t workspace_bytes, void* stream);

int g4s_mesh_compact_emit(int n_vertices, int n_triangles, const float* vertices, const float* vertex_colors,
                          const int* triangles, int compact_vertices, float* vertices_out, float* vertex_colors_out,
                          int* triangles_out, int n_vertices_out, int n_triangles_out, char* workspace,
                          size_t workspace_bytes, void* stream);

/* =====================================================================================================================
 * Mesh evaluation (g4splat_amd/csrc/tsdf/mesh_eval.hip).
 *
 * What the reference's eval/mesh_eval.py asks of scikit-learn's KDTree, open3d's VoxelDownSample and trimesh's
 * sample_surface before it forms accuracy, completeness, Chamfer-L1, precision, recall, F-score and normal consistency
 * (g4splat_amd/mesh_eval.py forms them).  The semantics below are this library's own, stated exactly
 * (tests/mesh_eval_ref.py restates them in numpy).  Clouds are [n,3] float32 device pointers with 3 n below 2^31.
 * Every output is a pure function of the input arrays; no atomics are used.
 *
 * A. Nearest neighbour.  For query q and reference index j: d(j) = ((x_j - q_x)^2 + (y_j - q_y)^2) + (z_j - q_z)^2 in
 *   float32, separate multiplies and adds in this association (g4s_knn_mean_dist's distance).  A candidate whose d is NaN
 *   or +inf never wins.  dist2_out[q] = the smallest d, index_out[q] = the smallest j that attains it; if no candidate
 *   is finite -- which includes a query with a non-finite coordinate -- FLT_MAX and -1.  The minimum and the tie rule are
 *   properties of the two clouds, so every exact search returns these bits.  n_query == 0 succeeds without a launch;
 *   n_ref <= 0 is an error (there is nothing to be nearest to).
 * B. Voxel down-sample (open3d's VoxelDownSample, with a defined order), two-phase.  lo = the per-axis minimum of the
 *   cloud minus voxel_size / 2, in float32.  Cell of a coordinate p: floor(((double)p - (double)lo) / (double)voxel_size),
 *   all in float64.  An output point is the sum of its voxel's points in float64 in ascending input index, divided by
 *   their count, rounded once to float32.  Voxels come out in ascending (cz, cy, cx).  count: *n_voxels (host int; one
 *   host synchronisation); emit, same n, points and workspace, the workspace untouched in between: points_out
 *   [n_voxels,3]; nothing is written beyond n_voxels.  Limit: with cells_a = the cell of the axis maximum + 1, the product
 *   cells_x cells_y cells_z - 1 and n - 1 must together fit 64 bits (cell bits + index bits <= 64), otherwise count
 *   returns G4S_ERR_INVALID_ARGUMENT and says so; so does a non-finite point (checked on the device, reported by count)
 *   and a voxel_size that is not finite and positive.  One thread sums a voxel: a cloud inside one voxel is summed
 *   serially.
 * C. Surface sampling (trimesh's sample_surface and face_normals, the random numbers passed in).  u [n_samples,3] float32
 *   in [0,1), cum_area [n_triangles] float64 = the inclusive running sum of the face areas (the caller's; non-decreasing).
 *   face = min(#{i : cum_area[i] <= (double)u0 * cum_area[n_triangles - 1]}, n_triangles - 1), i.e. searchsorted with
 *   side = 'right': a face of zero area is never chosen.  a = u1, b = u2; if a + b > 1 (float32): a = 1 - a, b = 1 - b.
 *   point = v0 + (a * (v1 - v0) + b * (v2 - v0)) in float32, this association, no contraction.  normal = c / len with
 *   c = (v1 - v0) x (v2 - v0) (each component one product minus the other) and len = sqrtf((cx^2 + cy^2) + cz^2); len == 0
 *   gives a zero normal.  A face that names a vertex outside [0, n_vertices) gives a NaN point and a zero normal.
 * Differences from the reference's libraries: points are float32 (open3d and trimesh work in float64); the down-sample
 * has an order (open3d's is a hash map's); the random numbers are the caller's, not numpy's global state; the sampler
 * uses side = 'right'; an empty reference cloud is an error (the reference returns NaN figures).
 * Every argument is checked on the host before anything is launched.
 */

/* Bytes of device workspace of g4s_nn_search: the reference cloud's tree and the queries' curve order. */
size_t g4s_nn_workspace(int n_ref, int n_query);

/* dist2_out [n_query] float32, index_out [n_query] int32. */
int g4s_nn_search(int n_ref, const float* ref, int n_query, const float* query, float* dist2_out, int* index_out,
                  char* workspace, size_t workspace_bytes, void* stream);

size_t g4s_voxel_downsample_workspace(int n);

int g4s_voxel_downsample_count(int n, const float* points, float voxel_size, int* n_voxels, char* workspace,
                               size_t workspace_bytes, void* stream);

int g4s_voxel_downsample_emit(int n, const float* points, int n_voxels, float* points_out, char* workspace,
                              size_t workspace_bytes, void* stream);

/* points_out, normals_out [n_samples,3] float32, face_out [n_samples] int32. */
int g4s_mesh_sample_surface(int n_samples, const float* u, const double* cum_area, int n_triangles, const int* triangles,
                            int n_vertices, const float* vertices, float* points_out, float* normals_out, int* face_out,
                            void* stream);

/* =====================================================================================================================
 * Visibility grid (g4splat_amd/csrc/tsdf/visibility.hip).
 *
 * The stage the reference puts between training and inpainting (2d-gaussian-splatting/render_novel_views.py,
 * guidance/vis_grid.py VisibilityGrid, guidance/cam_utils.py project_points_to_image / check_valid_camera_center_by_depth /
 * build_visibility_masks, planes/get_global_3Dpnts.py get_visible_mask_for_input_views): which voxels of the scene's box
 * some input view sees in free space, which pixels of a candidate view look only through such voxels, and how many views
 * confirm a point.  As above, the semantics are this library's own, stated exactly (tests/visibility_ref.py restates them
 * in numpy): float32, round-to-nearest-even, correctly rounded /, no fused multiply-add except the one named below,
 * evaluated left to right as written; min / max are IEEE minNum / maxNum (a NaN operand yields the other one).
 *
 * Views.  V views.  View v has world_view_transform Wv (16 floats, row-major, row-vector convention: M[r][c] = M[4r + c]),
 *   focal = {fx, fy} and a depth map [H,W], a float32 device pointer; W and H may differ between views (sizes = {W0, H0,
 *   W1, H1, ...}) and are the map's, whatever the camera says.  fx = W / (2 tan(FoVx / 2)), fy = H / (2 tan(FoVy / 2)), computed
 *   by the caller in double and rounded to float.
 * Projection of a point p into a view:  c_j = ((p0*Wv[0][j] + p1*Wv[1][j]) + p2*Wv[2][j]) + Wv[3][j] for j = 0, 1, 2; z = c_2;
 *   u = (c_0 / z) * fx + W/2, v = (c_1 / z) * fy + H/2 (W/2 = float(W) * 0.5, exact).  in image iff u >= 0 && u < W &&
 *   v >= 0 && v < H (every comparison with a NaN is false).  The tap is nearest by truncation:
 *   d = depth[min(int(v), H - 1)][min(int(u), W - 1)]; it is read only when the point is in the image.
 * Predicates per (point, view):  FREE (mode 0) = in image && z > 0 && z < d.  SURFACE (mode 1) = in image && z > 0 &&
 *   |z - d| / (z + 1e-6) < depth_threshold.
 * Grid.  resolution R >= 1, R^3 < 2^31, over the box bbox_min .. bbox_max (3 host floats each, finite, max > min on every
 *   axis).  extent = bbox_max - bbox_min and grid_size = extent / float(R) per axis.  The centre of voxel (ix, iy, iz) is
 *   bbox_min + (float(i) + 0.5) * grid_size per axis; its flat index is (ix * R + iy) * R + iz, z fastest.  A voxel is
 *   visible iff some view passes FREE at its centre.  Storage: ceil(R^3 / 64) 64-bit words, bit (flat & 63) of word
 *   (flat >> 6); the bits beyond R^3 are zero.  No atomics: every word is written once.
 * Point -> voxel:  per axis i = int(min(max(((p - bbox_min) / extent) * float(R), 0), float(R - 1))), clamped as a float and
 *   then truncated.  A point outside the box lands in a border voxel (the reference's behaviour); a NaN coordinate gives
 *   index 0 (stated here; the reference leaves it undefined).
 * Ray record of a camera:  twelve host floats, origin o[3] then D[3][3] row-major.  For integer pixel coordinates (x, y),
 *   no half-pixel offset: dir_r = (D[r][0]*x + D[r][1]*y) + D[r][2], and the point at parameter t is o_r + t * dir_r.  The
 *   caller computes the record in double (c2w = inverse of Wv^T; D = c2w[:3,:3] times the inverse of the pixel intrinsics
 *   the reference derives from full_proj_transform and the map's size; o = c2w[:3,3]) and rounds it to float.
 * Back-projection of a depth map [H,W]:  pixel i = y * W + x with depth q gives the point o_r + q * dir_r.
 * Ray march of a depth map [H,W] with n_samples = S >= 1:  a pixel with depth <= 1e-6 is invalid and gets 0.  Any other
 *   pixel with depth q gets 1 iff for every k in [0, S - 10) the voxel of the point at t = t_k * q is visible, else 0;
 *   S <= 10 means no sample, every valid pixel gets 1.  t_k is element k of torch.linspace(0, 1, S) in float32:
 *   step = 1 / float(S - 1); t_k = step * float(k) for k < S / 2 (integer division), otherwise
 *   t_k = fma(-step, float(S - 1 - k), 1), a single rounding -- the one fused operation of this section, because torch's
 *   kernel fuses it.  The caller chooses S; the reference's is int(m / min(grid_size)) + 1 with m the largest depth after
 *   every invalid pixel was replaced by 1e-3.  The depth map is only read (the reference overwrites its invalid pixels).
 * Compaction.  The centres of the visible (invisible != 0: of the invisible) voxels in ascending flat index, two-phase:
 *   compact_count reads back their number (one host synchronisation); compact_emit, same resolution, words, `invisible`
 *   and workspace, the workspace untouched in between, writes centres [n_points,3] and nothing beyond n_points.
 * View counts.  counts[i] = the number of views v != skip_view (-1: none is skipped) that pass the predicate of `mode` at
 *   point i -- an explicit point, or pixel i of pixel_depth back-projected with `ray`.
 *
 * world_view [V,16], focal [V,2], sizes [V,2] and the array of V map pointers are HOST arrays, read during the call (the
 * library packs them into a table in the workspace, g4s_visgrid_workspace(V) bytes).  Every argument is checked on the
 * host before anything is launched.  Every entry point takes workspace, workspace_bytes; those that name no size query use
 * none and accept NULL, 0.
 */

/* Bytes of device workspace of g4s_visgrid_build / g4s_view_counts_points / g4s_view_counts_pixels for n_views views. */
size_t g4s_visgrid_workspace(int n_views);

/* words [ceil(resolution^3 / 64)]: the packed grid, every word written once.  n_views = 0: all zero. */
int g4s_visgrid_build(int resolution, const float* bbox_min, const float* bbox_max, int n_views, const float* world_view,
                      const float* focal, const int* sizes, const float* const* depth, unsigned long long* words,
                      char* workspace, size_t workspace_bytes, void* stream);

/* visible [n_points]: 1 iff the voxel of points [n_points,3] (device) is visible. */
int g4s_visgrid_sample(int resolution, const float* bbox_min, const float* bbox_max, const unsigned long long* words,
                       int n_points, const float* points, unsigned char* visible, char* workspace, size_t workspace_bytes,
                       void* stream);

/* visibility [height,width] float32, 0 or 1: the ray march of depth [height,width] with the ray record `ray`. */
int g4s_visgrid_march(int resolution, const float* bbox_min, const float* bbox_max, const unsigned long long* words,
                      int width, int height, const float* depth, const float* ray, int n_samples, float* visibility,
                      char* workspace, size_t workspace_bytes, void* stream);

/* The same march over a grid of one byte per voxel [resolution^3] (non-zero = visible) in flat-index order: the storage
 * the packed words are measured against (tools/bench_visibility.py); the results are the same. */
int g4s_visgrid_march_bytes(int resolution, const float* bbox_min, const float* bbox_max, const unsigned char* grid,
                            int width, int height, const float* depth, const float* ray, int n_samples, float* visibility,
                            char* workspace, size_t workspace_bytes, void* stream);

/* grid [resolution^3] float32, 0 or 1 in flat-index order: the reference's `visibility_grid`. */
int g4s_visgrid_expand(int resolution, const unsigned long long* words, float* grid, char* workspace, size_t workspace_bytes,
                       void* stream);

/* Bytes of device workspace of the compaction (0 for a resolution outside the grid's range). */
size_t g4s_visgrid_compact_workspace(int resolution);

int g4s_visgrid_compact_count(int resolution, const unsigned long long* words, int invisible, int* n_points,
                              char* workspace, size_t workspace_bytes, void* stream);

int g4s_visgrid_compact_emit(int resolution, const float* bbox_min, const float* bbox_max, const unsigned long long* words,
                             int invisible, int n_points, float* centres, char* workspace, size_t workspace_bytes,
                             void* stream);

/* counts [n_points] int32 for points [n_points,3] (device). */
int g4s_view_counts_points(int n_points, const float* points, int mode, float depth_threshold, int skip_view, int n_views,
                           const float* world_view, const float* focal, const int* sizes, const float* const* depth,
                           int* counts, char* workspace, size_t workspace_bytes, void* stream);

/* counts [height,width] int32 for the pixels of pixel_depth [height,width] back-projected with `ray`. */
int g4s_view_counts_pixels(int width, int height, const float* pixel_depth, const float* ray, int mode,
                           float depth_threshold, int skip_view, int n_views, const float* world_view, const float* focal,
                           const int* sizes, const float* const* depth, int* counts, char* workspace, size_t workspace_bytes,
                           void* stream);

/* points [height * width,3]: the back-projection of depth [height,width] with `ray`. */
int g4s_depth_to_points(int width, int height, const float* depth, const float* ray, float* points, char* workspace,
                        size_t workspace_bytes, void* stream);

/* =====================================================================================================================
 * Global planes (g4splat_amd/csrc/tsdf/planes.hip).
 *
 * The stage the reference puts between view selection and plane-aware depth refinement (2d-gaussian-splatting/
 * planes/merge_global_3Dplane.py get_global_3Dplane over guidance/cam_utils.py get_pixel_to_points_tensor): which points of
 * a chart cloud each view's plane mask claims, and which local planes of which views are one scene plane.  The library
 * computes labels, the membership of points in global planes and integer counts; the sequential merge decisions are the
 * caller's (g4splat_amd/planes.py), on the host, over those counts.  The semantics are this library's own, stated exactly
 * (tests/planes_ref.py restates them in numpy): float32, round-to-nearest-even, correctly rounded /, no fused
 * multiply-add, evaluated left to right as written.
 *
 * Views.  As in the Visibility section, with the view's map being its slot mask [H,W], an int32 device pointer whose values
 *   are 0 (no plane) .. P (the caller remaps arbitrary mask ids to slots); W and H are the mask's, whatever the camera
 *   says.  c_j, z, u, v and "in image" are the Visibility section's projection, the same device function.
 * Candidates.  Point i of points [N,3] is a candidate of a view iff i != 0 && in image && z > 0 (index 0 is the reference's
 *   "empty slot" and is never a member of anything).  Its pixel is px = min(int(rint(u)), W - 1), py = min(int(rint(v)),
 *   H - 1), rint rounding half to even.
 * Front points.  zmin[py][px] = the minimum of z over the view's candidates of that pixel, taken as an unsigned integer
 *   atomic min of the floats' bit patterns (z > 0: the bits order like the values), so it does not depend on the order of
 *   execution.  label[i] = mask[py][px] if i is a candidate and z < zmin[py][px] + depth_thresh (one float32 add, strict <),
 *   otherwise 0.  depth_thresh < 0 turns the depth test off (the reference's use_depth_threshold=False): every candidate
 *   takes its pixel's mask value.  A point has at most one label per view: the local planes S_p = {i : label[i] = p} of a
 *   view are disjoint.
 * Membership.  G global planes, n_words >= ceil(G / 64) 64-bit words per point: bit (g & 63) of member[(g >> 6) * N + i] says
 *   that point i belongs to global plane g (point-major words, stored one block of N words per 64 planes; the caller
 *   grows it by whole blocks and keeps the bits at and above G zero).  Row g = {i : that bit is set}.
 * Overlap.  counts[(p - 1) * G + g] = |S_p ∩ row g| and sizes[p - 1] = |S_p| for p = 1 .. P; labels outside 1 .. P count as
 *   0.  Integer sums by integer atomics: exact and independent of the order.  There is no float atomic in this section.
 * Assign.  target[p - 1] (host, P ints) is -1 or a global plane below G: every point with label p gets that bit.
 * Row overlap.  counts[h] = |row ∩ row h| for h < G; counts[row] is the row's size.
 * Row merge.  Every point of row src joins row dst.   Row mask.  mask[i] = 1 iff point i is in the row, else 0; the
 *   ascending indices of a row are the non-zero positions of its mask.
 *
 * Memory.  Labels are int32 [V,N] for the V views of one call, the workspace holds the view table (88 bytes per view) and one
 *   zmin word per mask pixel; the caller chunks a long view list.  At N = 5 * 10^6: 20 MB of labels per view (1.2 GB if all
 *   60 views are labelled in one call), 40 MB of membership per 64 global planes.
 *
 * Differences from the reference, on purpose.  No cap of 500 points per pixel (the reference drops the excess in an order
 *   its unstable sort leaves undefined).  The mask's size stands in for the camera's.  The dense [H,W,K] pixel-to-points
 *   map is not offered; labels carry the same information.  An empty global plane (the reference makes one from a view-0
 *   mask id without front points and later divides by its size) has rate 0 against everything in the caller's decisions.
 *   A decision at an edge -- a point on the image border, a u or v at .5, z at zmin + depth_thresh -- is made in this
 *   section's float32 order, which is not torch's matmul order; the tests compare on the set where float32 and float64
 *   agree.
 *
 * world_view [V,16], focal [V,2], sizes [V,2], the array of V mask pointers and `target` are HOST arrays, read during the
 * call.  Every argument is checked on the host before anything is launched.  Every entry point takes workspace,
 * workspace_bytes; those that name no size query use none and accept NULL, 0.
 */

/* Bytes of device workspace of g4s_plane_labels for views of these sizes (0 for sizes out of range). */
size_t g4s_plane_labels_workspace(int n_views, const int* sizes);

/* labels [n_views, n_points] int32 for points [n_points,3] (device).  n_views = 0: nothing is written. */
int g4s_plane_labels(int n_points, const float* points, float depth_thresh, int n_views, const float* world_view,
                     const float* focal, const int* sizes, const int* const* masks, int* labels, char* workspace,
                     size_t workspace_bytes, void* stream);

/* counts [n_planes * n_global] and sizes [n_planes] uint32 (device), cleared and filled; labels [n_points] of one view. */
int g4s_plane_overlap(int n_points, const int* labels, int n_planes, int n_global, int n_words,
                      const unsigned long long* member, unsigned int* counts, unsigned int* sizes, char* workspace,
                      size_t workspace_bytes, void* stream);

/* Bytes of device workspace of g4s_plane_assign. */
size_t g4s_plane_assign_workspace(int n_planes);

int g4s_plane_assign(int n_points, const int* labels, int n_planes, const int* target, int n_global, int n_words,
                     unsigned long long* member, char* workspace, size_t workspace_bytes, void* stream);

/* counts [n_global] uint32 (device), cleared and filled. */
int g4s_plane_row_overlap(int n_points, int n_global, int n_words, const unsigned long long* member, int row,
                          unsigned int* counts, char* workspace, size_t workspace_bytes, void* stream);

int g4s_plane_row_merge(int n_points, int n_global, int n_words, unsigned long long* member, int src, int dst,
                        char* workspace, size_t workspace_bytes, void* stream);

/* mask [n_points] bytes (device). */
int g4s_plane_row_mask(int n_points, int n_global, int n_words, const unsigned long long* member, int row,
                       unsigned char* mask, char* workspace, size_t workspace_bytes, void* stream);

/* =====================================================================================================================
 * Cross-view consistency (g4splat_amd/csrc/tsdf/consistency.hip).
 *
 * The third stage the reference runs between view selection and training (scripts/plane_refine_depth.py): one of two
 * "inconsistency solvers", 2d-gaussian-splatting/guidance/inconsistence_solver.py (points) or guidance/
 * plane_inconsistency_solver.py (planes), writes the confident maps train_with_refine_depth.py loads and repaints the
 * inpainted images so that views agree on colour.  The semantics are this library's own, stated exactly
 * (tests/consistency_ref.py restates them in numpy): float32, round-to-nearest-even, correctly rounded /, no fused
 * multiply-add, evaluated left to right as written.
 *
 * Views.  As in the Visibility section: world_view, focal, sizes, a depth map [H,W] per view.  W and H are the depth map's;
 *   every image, mask, confident map and point grid of a view has that size.  The projection, "in image", the truncating
 *   tap and SURFACE are that section's, the same device functions.  vis(p, v) = SURFACE of point p in view v with
 *   depth_threshold; pix(p, v) = the row-major index of its tap, min(int(v), H - 1) * W + min(int(u), W - 1).
 *
 * A. Point solver.  V views, the first I = n_input_views of them input views, the others inpainted views.  images[v] is float32,
 *   [H,W,3] (image_chw[v] = 0) or [3,H,W] (image_chw[v] != 0), values in 0 .. 1.  points [N,3] float32 (device), N < 2^31.
 *   seen(i) = vis(i, v) for some v < I.  visible(i) = vis(i, v) for some v < V.  For a point that is visible and not seen:
 *   first(i) = the smallest v with vis(i, v) and colour(i)[c] = uint8(trunc(images[first][pix(i, first)][c] * 255.0f)) (a
 *   product outside 0 .. 255 is clamped to that range first, a NaN gives 0).  images are only ever read; outputs are
 *   separate buffers.
 *   conf[v] [H,W] uint8 = 1 everywhere, except 0 at pix(i, v) of every i with v >= I, vis(i, v) and seen(i).
 *   images_out[v] [H,W,3] float32 = images[v] (in [H,W,3] order), except that at every pixel that is pix(i, v) of at least
 *   one i with v >= I, vis(i, v) and not seen(i), channel c becomes float(colour(w)[c]) / 255.0f, w being the LARGEST such
 *   point index (an integer atomic max per pixel: independent of the order of execution).  An input view keeps conf = 1
 *   and its image.
 *   state [N] uint32: bits 0 .. 7, 8 .. 15, 16 .. 23 = colour(i)[0 .. 2] (0 unless visible and not seen), bit 24 = seen(i),
 *   bit 25 = visible(i).  With resume != 0 the kernel starts from the state of an earlier call over EARLIER views of the
 *   same list, so a caller may pass a long list in chunks: every chunk of input views before the first chunk with an
 *   inpainted view, in the list's order; the outputs of a chunk's views are final when its call returns.
 *   images_out and conf may both be NULL: no outputs, the state alone.  state may be NULL when no inpainted view needs
 *   it (I = V, or N = 0); then, and with N = 0, nothing is launched beyond the fills of conf and images_out.
 *   Storage: 4 bytes per point (state) and 4 bytes per pixel of the inpainted views (the workspace's winner words),
 *   nothing per (point, view) pair; the view table takes 120 bytes per view.
 *
 * B. Plane solver.  Per view a uint8 image [H,W,3], a slot mask [H,W] int32 and pixel-aligned points [H*W,3] float32, all
 *   device pointers.  The caller remaps arbitrary mask ids to slots 0 (no plane) .. P_v per view and flattens per-slot
 *   tables: view v owns entries slot_offset[v] .. slot_offset[v + 1] - 1 (slot_offset [V + 1], slot_offset[0] = 0, at least
 *   slot 0 per view; entry slot_offset[v] + s belongs to slot s; a mask value outside the view's slots counts as slot 0,
 *   whose entries are -1).
 *   Counts.  slot_plane[e] = the global plane k < n_planes of the slot, or -1.  counts[k * n_anchors + j] = the number of
 *   pixels q of all views w whose slot names plane k and whose point points[w][q] passes SURFACE in view anchor_views[j].
 *   Integer sums by integer atomics, folded across the wave first.  The anchor of a plane is the caller's decision.
 *   Repaint.  slot_step[e] = the step t >= 0 of the slot's (view, plane) pair, or -1; slot_anchor[e] = the anchor view a of
 *   its plane.  For pixel x = (w, q) whose slot has a step and whose point passes SURFACE in a: step(x) = t, src(x) = (a,
 *   pix(points[w][q], a)).  Every other pixel has step(x) = infinity.  images_out[w][q] = value(x, infinity) with
 *   value(x, T) = value(src(x), step(x)) if step(x) < T, otherwise images[view of x][pixel of x].  Steps strictly decrease
 *   along a chain, so the walk ends.  This is exactly what repainting the images in place, step after step, the right-hand
 *   side of a step evaluated before it is assigned, leaves behind: a read from an image that an EARLIER step repainted sees
 *   the repainted colour, a read inside the same step (w = a) sees the state before the step.  images are only read.
 *   Storage: 12 bytes per pixel of the views in the workspace (step, source view, source pixel), 128 bytes per view; the
 *   views of one call have fewer than 2^31 pixels in all.
 *
 * Differences from the reference, on purpose.  Duplicate pixels of the point solver resolve to the largest point index (the
 *   reference leaves the winner to index_put, undefined on a GPU; a single-threaded CPU run writes in index order, which is
 *   this rule).  A decision at an edge -- a point on the image border, a u or v on an integer, a relative difference exactly
 *   at the threshold -- is made in this section's float32 order, which is not torch's matmul order.  The [N,V] visibility
 *   and coordinate tables are not offered.  There is no file I/O: the callers keep writing PNGs, the all-ones pseudo
 *   confident maps of the plane solver and of the no-inpainting branch included.  The reference's unused color_eps is
 *   dropped.  A point that no view sees has colour 0 (the reference gives it view 0's pixel (0, 0) and never uses it).
 *
 * world_view, focal, sizes, image_chw, the pointer arrays, slot_offset, slot_plane, slot_step, slot_anchor and anchor_views
 * are HOST arrays, read during the call.  At most 65535 views per call.  Every argument is checked on the host before
 * anything is launched.  Every entry point takes workspace, workspace_bytes.
 */

/* Bytes of device workspace of g4s_consistency_points for views of these sizes (0 for arguments out of range). */
size_t g4s_consistency_points_workspace(int n_views, int n_input_views, const int* sizes);

int g4s_consistency_points(int n_points, const float* points, float depth_threshold, int n_views, int n_input_views,
                           const float* world_view, const float* focal, const int* sizes, const float* const* depth,
                           const float* const* images, const int* image_chw, float* const* images_out,
                           unsigned char* const* conf, int resume, unsigned int* state, char* workspace,
                           size_t workspace_bytes, void* stream);

/* Bytes of device workspace of g4s_consistency_plane_counts; n_slots = slot_offset[n_views]. */
size_t g4s_consistency_plane_counts_workspace(int n_views, int n_slots, int n_anchors);

/* counts [n_planes * n_anchors] uint32 (device), cleared and filled. */
int g4s_consistency_plane_counts(float depth_threshold, int n_views, const float* world_view, const float* focal,
                                 const int* sizes, const float* const* depth, const int* const* masks,
                                 const float* const* points, const int* slot_offset, const int* slot_plane, int n_planes,
                                 int n_anchors, const int* anchor_views, unsigned int* counts, char* workspace,
                                 size_t workspace_bytes, void* stream);

/* Bytes of device workspace of g4s_consistency_plane_repaint (0 for arguments out of range). */
size_t g4s_consistency_plane_repaint_workspace(int n_views, const int* sizes, int n_slots);

int g4s_consistency_plane_repaint(float depth_threshold, int n_views, const float* world_view, const float* focal,
                                  const int* sizes, const float* const* depth, const int* const* masks,
                                  const float* const* points, const unsigned char* const* images,
                                  unsigned char* const* images_out, const int* slot_offset, const int* slot_step,
                                  const int* slot_anchor, char* workspace, size_t workspace_bytes, void* stream);

/* =====================================================================================================================
 * View selection (g4splat_amd/csrc/tsdf/view_select.hip).
 *
 * The two device pieces of the reference's novel-view stage that sit between the visibility maps and the camera file
 * (2d-gaussian-splatting/render_novel_views.py over guidance/cam_utils.py): select_need_inpaint_views, which asks
 * covisibility_check_by_gs for pairs of candidate cameras, and get_novel_cams_lookat_points, which runs
 * farthest_point_sample once per input view.  The library computes bits, integer counts and samples; the sequential
 * decisions and the random draws are the caller's (g4splat_amd/view_selection.py).  The semantics are this library's own,
 * stated exactly (tests/view_selection_ref.py restates them in numpy): float32, round-to-nearest-even, correctly rounded /,
 * no fused multiply-add, evaluated left to right as written; min is IEEE minNum.
 *
 * A. Visible bits and the covisibility table.  C >= 1 cameras, at most 65535, each with world_view, focal and sizes as in
 *   the Visibility section; a camera here has a size {W, H} but no map.  points [P,3] float32 (device), 0 <= P <= 2^31 - 64.
 *   Camera c sees point p iff in image && z > 0, with c_j, z, u, v and "in image" the Visibility section's projection, the
 *   same device function (every comparison with a NaN is false: a point with a NaN coordinate is seen by no camera).
 *   words [C, ceil(P / 64)] 64-bit: bit (p & 63) of words[c][p >> 6] is set iff camera c sees point p; the bits beyond P
 *   are zero.  Every word is written once, no atomics.
 *   counts [C,C] int32: counts[i][j] = sum over w of popcount(words[i][w] & words[j][w]), the number of points both
 *   cameras see; the diagonal holds the visible counts, the matrix is symmetric.  Integer sums by integer atomics: the
 *   result does not depend on the order of execution.  n_words = 0 gives zero counts and launches nothing.
 *   The overlap takes any words [C, n_words] of that layout (n_words <= 2^25); it does not look at P.
 *
 * B. Farthest-point sampling, batched.  clouds [M,N,3] float32 (device), finite; 1 <= M <= 65535, 3 <= N <= 2^30; k samples
 *   with 2 <= k < N and M k <= 2^30; first [M] (HOST) the index of each cloud's sample 0, 0 <= first[m] < N.
 *   Per cloud: dist_0[n] = 1e10f.  For round i = 1 .. k - 1, with q the point chosen in round i - 1 (round 0: first):
 *   dx = p_n.x - q.x, dy, dz alike; d[n] = (dx*dx + dy*dy) + dz*dz; dist_i[n] = min(dist_{i-1}[n], d[n]); the choice of round i
 *   is the n of largest dist_i[n], the SMALLEST such n on ties (the key (bits of dist_i[n] << 32) | ~n, dist >= 0, taken by a
 *   64-bit unsigned atomic max: independent of the order of execution).
 *   indices [M,k] int32; samples [M,k,3] = the chosen points; dist [M,N] = dist_{k-1}, required: it is the running minimum
 *   the rounds work on.  k launches for all clouds together (k - 1 rounds and the gather).  The behaviour for non-finite
 *   coordinates is unspecified beyond memory safety (every index stays inside its cloud).
 *
 * world_view, focal, sizes and first are HOST arrays, read during the call.  Every argument is checked on the host before
 * anything is launched.  Every entry point takes workspace, workspace_bytes; those that name no size query use none and
 * accept NULL, 0.
 */

/* Bytes of device workspace of g4s_view_bits for n_views cameras (the view table, 80 bytes per camera). */
size_t g4s_view_bits_workspace(int n_views);

/* words [n_views, ceil(n_points / 64)] for points [n_points,3] (device).  n_points = 0: nothing is launched. */
int g4s_view_bits(int n_points, const float* points, int n_views, const float* world_view, const float* focal,
                  const int* sizes, unsigned long long* words, char* workspace, size_t workspace_bytes, void* stream);

/* counts [n_views, n_views] int32 (device), cleared and filled from words [n_views, n_words]. */
int g4s_view_overlap(int n_views, int n_words, const unsigned long long* words, int* counts, char* workspace,
                     size_t workspace_bytes, void* stream);

/* Bytes of device workspace of g4s_fps (0 for arguments out of range). */
size_t g4s_fps_workspace(int n_clouds, int n_samples);

int g4s_fps(int n_clouds, int n_points, const float* clouds, const int* first, int n_samples, int* indices, float* samples,
            float* dist, char* workspace, size_t workspace_bytes, void* stream);

/* =====================================================================================================================
 * Depth cues (g4splat_amd/csrc/tsdf/depth_cues.hip).
 *
 * What the reference does to every inpainted view between the inpainter and the global-plane merge (2d-gaussian-splatting/
 * guidance/see3d_dn_util.py, guidance/dense_dn_util.py: visibility, matcha/pointmap/depthanythingv2.py depth_linear_align,
 * utils/point_utils.py depth_to_normal, the merge) and between the merge and the inconsistency solvers (planes/
 * refine_depth_with_planes.py: compute_plane_aligned_depth pasted per (plane, view) pair, the second alignment, the refill).
 * The plane FIT stays with the caller: fitted planes are an input.  The semantics are this library's own, stated exactly
 * (tests/depth_cues_ref.py restates them in numpy): float32 unless float64 is named, round-to-nearest-even, correctly
 * rounded / and sqrt, no fused multiply-add anywhere in this section, evaluated left to right as written; max is IEEE maxNum.
 *
 * Views.  V views, at most 65535 per call, sizes = {W0, H0, W1, H1, ...}, W H <= 2^30; the maps of view v are device pointers
 *   to [H_v, W_v] arrays, passed as HOST arrays of V pointers.  Pixel q = y W + x.
 *
 * A. Alignment.  Per view a source map s, a target map g and a mask: uint8 [H,W], set iff non-zero, or (mask_is_map != 0) a
 *   float32 map, set iff value > mask_threshold.  Per masked pixel, by `domain`:
 *     0 (disparity)       t = 1 / g,  d = s          -- depth_linear_align
 *     1 (depth)           t = g,      d = s          -- depth_linear_align_2
 *     2 (inverse source)  t = 1 / g,  d = 1 / s      -- depth_linear_align of the disparity 1 / s, which is never stored
 *   t and d are float32.  n = the number of masked pixels; St, Sd, Std, Sdd = the sums of t, d, t d, d d over them in
 *   float64 (a product of two float32 values is exact there).  The order of the additions is fixed: a workgroup owns
 *   G4S_DEPTH_ALIGN_SPAN consecutive pixels, a thread adds its pixels in ascending order, a fixed tree folds the threads, and
 *   the workgroups' partials are added by index.  No floating-point atomics: two runs give the same bits.  Then, in float64,
 *     beta = (Std - St Sd / n) / (Sdd - Sd Sd / n),   alpha = (St - beta Sd) / n,
 *   both rounded to float32: coeffs[v] = {alpha, beta}, counts[v] = n (int32), both on the device.  A degenerate view
 *   (n = 0, n = 1, no variance of d, a masked g = 0) gives what IEEE arithmetic gives: NaN or inf.  That is no error.
 *   aligned(s) = 1 / (alpha + beta d) with d as above (domain 0, 2), alpha + beta d (domain 1): one multiplication, one
 *   addition, one division, each rounded.
 *   g4s_depth_align: 2 launches.  g4s_depth_align_apply: 1 launch.
 *
 * B. Cue maps of view v with coeffs[v] = {alpha, beta}, mono disparity d, rendered ("warp") depth and alpha map, 1 launch:
 *   visibility = alpha_map > visible_threshold (uint8 0 / 1);  mono_depth = 1 / d;  aligned_depth = aligned(d), domain 0;
 *   merged_depth = visibility ? warp_depth : aligned_depth.
 *   normal_world [H,W,3]: 0 on the one-pixel border (so everywhere if W < 3 or H < 3).  Elsewhere P(x, y) = the back-
 *   projection of the Visibility section (the same device function as g4s_depth_to_points) of pixel (x, y) with the view's
 *   ray record at depth aligned(d(x, y)) -- recomputed from the neighbour's disparity, no finished map is read --;
 *   dx = P(x, y + 1) - P(x, y - 1), dy = P(x + 1, y) - P(x - 1, y); n = dx x dy, n_0 = dx_1 dy_2 - dx_2 dy_1 and cyclic (two
 *   rounded products, one subtraction); len = max(sqrt((n_0 n_0 + n_1 n_1) + n_2 n_2), 1e-12); normal_world = n / len.
 *   normal_cam_j = (nw_0 Wv[0][j] + nw_1 Wv[1][j]) + nw_2 Wv[2][j], Wv = world_view_transform, row-major.
 *   rays [V,12] are the views' ray records, world_view [V,16]: HOST arrays.
 *
 * C. Plane depths, 1 launch (and one memset of the counts).  cameras [V,14] (HOST): o[3] the camera centre, R[3][3] the
 *   camera -> world rotation row-major (both from the inverse of world_view_transform, taken by the caller in double),
 *   fx = W / (2 tan(FoVx / 2)), fy alike.  planes [P,6] (HOST, finite): normal n[3], centre c[3].  The table of fitted
 *   (view, id) pairs: view v owns entries view_offset[v] .. view_offset[v + 1] - 1 (view_offset [V + 1], view_offset[0] = 0);
 *   ids[e] > 0, strictly ascending inside a view; entry_plane[e] < P.  The caller builds it from global_3Dplane_ID_dict: a pair
 *   listed under several fitted planes keeps the last in dict order, a pair whose plane was not fitted has no entry.
 *   A pixel whose mask value (int32, any positive ids) has an entry with plane (n, c):
 *     dcx = (float(x) - W/2) / fx, dcy = (float(y) - H/2) / fy (W/2 = float(W) * 0.5, exact);
 *     w_r = (R[r][0] dcx + R[r][1] dcy) + R[r][2];  len = max(sqrt((w_0 w_0 + w_1 w_1) + w_2 w_2), 1e-12);  r = w / len;
 *     nd = (n_0 r_0 + n_1 r_1) + n_2 r_2;  nd' = copysign(max(|nd|, 1e-8), nd);
 *     num = (n_0 (c_0 - o_0) + n_1 (c_1 - o_1)) + n_2 (c_2 - o_2);  t = num / nd';  z = t / len
 *   (z is the camera-space depth of o + t r: R is a rotation, so |w| = |dc| and z = t / |dc|).  depth_out = z if t > 0 and
 *   z > 0, otherwise 0 -- the 0 is written, as the reference writes it.  Every other pixel: depth_out = depth.  depth_out[v]
 *   may be depth[v].  nd = 0 exactly is outside the compared contract (the reference's sign(0) = 0 divides by zero).
 *   counts [2,V] int32 (device), cleared and filled: counts[0][v] = pixels that took a z, counts[1][v] = pixels that took the
 *   0.  Integer sums, one integer atomic per wave.
 *
 * D. Refill, 1 launch.  For views v >= n_input_views, with coeffs[v] of A in domain 2 on (mono_depth, the plane-refined depth,
 *   the confident map): where mask == 0 and conf == 0, depth = aligned(mono_depth), domain 2, in place.  Nothing else is
 *   written; coeffs [V,2] is indexed by the view, the rows of the input views are not read.
 *
 * E. The refined points are g4s_depth_to_points of each refined map: one launch per view, nothing new.
 *
 * Differences from the reference, on purpose.  compute_plane_aligned_depth's second result, the list of valid points, is
 *   replaced by the validity the 0 encodes.  The focal lengths come from FoVx, FoVy and the map's size, not from the
 *   camera's focal_x, focal_y.  The sums are float64 in a fixed order (torch sums float32 in an order of its own), so alpha
 *   and beta are the correctly rounded least-squares coefficients to within one unit in the last place.  alpha is formed
 *   from the unrounded beta.
 *
 * Every argument is checked on the host before anything is launched.  The size queries are pure host code and return 0 for
 * arguments out of range.
 */
#define G4S_DEPTH_ALIGN_SPAN 4096 /* pixels per workgroup of the alignment sums */

size_t g4s_depth_align_workspace(int n_views, const int* sizes);

/* coeffs [n_views,2] float32 and counts [n_views] int32 (device). */
int g4s_depth_align(int domain, int mask_is_map, float mask_threshold, int n_views, const int* sizes,
                    const float* const* source, const float* const* target, const void* const* masks, float* coeffs,
                    int* counts, char* workspace, size_t workspace_bytes, void* stream);

size_t g4s_depth_align_apply_workspace(int n_views);

/* aligned[v] [H,W] = aligned(source[v]) with coeffs[v]. */
int g4s_depth_align_apply(int domain, int n_views, const int* sizes, const float* const* source, const float* coeffs,
                          float* const* aligned, char* workspace, size_t workspace_bytes, void* stream);

size_t g4s_depth_cue_maps_workspace(int n_views);

int g4s_depth_cue_maps(int n_views, const float* world_view, const float* rays, const int* sizes,
                       const float* const* disparity, const float* const* warp_depth, const float* const* alpha_map,
                       float visible_threshold, const float* coeffs, unsigned char* const* visibility,
                       float* const* mono_depth, float* const* aligned_depth, float* const* merged_depth,
                       float* const* normal_world, float* const* normal_cam, char* workspace, size_t workspace_bytes,
                       void* stream);

/* n_entries = view_offset[n_views]. */
size_t g4s_plane_depths_workspace(int n_views, int n_entries, int n_planes);

int g4s_plane_depths(int n_views, const float* cameras, const int* sizes, const float* const* depth,
                     float* const* depth_out, const int* const* masks, const int* view_offset, const int* ids,
                     const int* entry_plane, int n_planes, const float* planes, int* counts, char* workspace,
                     size_t workspace_bytes, void* stream);

size_t g4s_depth_refill_workspace(int n_views);

int g4s_depth_refill(int n_views, int n_input_views, const int* sizes, float* const* depth,
                     const float* const* mono_depth, const int* const* masks, const unsigned char* const* conf,
                     const float* coeffs, char* workspace, size_t workspace_bytes, void* stream);

/* =====================================================================================================================
 * Chart surfels (g4splat_amd/csrc/tsdf/chart_init.hip; the index pick is in mesh_eval.hip).
 *
 * The trainer's first act (2d-gaussian-splatting/train_with_refine_depth.py, "Initialize gaussians", the path that is not
 * the warp initialiser): the pixel grid of every view is triangulated (matcha/dm_scene/meshes.py
 * get_manifold_meshes_from_pointmaps), elongated faces are dropped (matcha/dm_scene/charts.py
 * get_gaussian_parameters_from_pa_data / _from_charts_data) and every surviving face carries one surfel
 * (matcha/dm_scene/gaussians.py get_gaussian_surfel_parameters_from_mesh with one barycentre); voxel_downsample_gaussians
 * then picks one surfel index per voxel.  tests/chart_init_ref.py restates this section in numpy.
 *
 * Views.  n_views views of height x width pixels, all of one size.  maps[v] is the point map [height,width,3]
 *   (depth_form == 0) or the depth map [height,width] (depth_form != 0); in depth form the point of pixel i = y * width +
 *   x is that of g4s_depth_to_points with rays[12 v .. 12 v + 11] (the Visibility section's ray record), computed in the
 *   kernel by the same arithmetic; the point map is never stored.  images[v] is [height,width,3] float32, masks[v]
 *   [height,width] uint8 (masks may be NULL: no mask).  Limit: 2 n_views (height-1)(width-1) < 2^31 and height * width
 *   < 2^31.
 *
 * Faces and their order.  Cell (r, c) of view v, r < height-1, c < width-1, has face_1 = (p[r,c], p[r+1,c], p[r,c+1]) and
 *   face_2 = (p[r+1,c+1], p[r,c+1], p[r+1,c]).  Order: all face_1 of view 0 in row-major cell order, all face_2 of view 0,
 *   then view 1, ...  Surviving faces keep this order: output row m is the m-th surviving face.  height == 1 or width == 1
 *   gives no face and succeeds with n_faces = 0.
 *
 * Keep test of a face (A, B, C).  float32, every operation rounded on its own (no contraction), this association:
 *   x.y = (x0 y0 + x1 y1) + x2 y2, |x| = sqrt(x.x), floor(t) = t if t > 1e-12f else 1e-12f (also for a NaN t).
 *   s0 = C - A, s1 = A - B, s2 = B - C;  n_i = s_i / floor(|s_i|) per component;
 *   a_i = s_i - (s_i . n_((i+1) mod 3)) n_i per component;  l_i = |a_i|.
 *   keep iff no l_i is a NaN and max(l) / min(l) < ratio_th (0 / 0 is a NaN: dropped; so is every face with a NaN or an
 *   infinite vertex, whose l are NaN).  This is the code of charts.py, whose comment describes a different quantity.
 *   Masks: iff masks is given and some byte of some view is non-zero (the reference's masks.any()), a face is also dropped
 *   unless at least ONE of its three vertices is masked in (remove_verts_from_single_mesh's any(dim=-1)).  An all-zero
 *   mask removes nothing.
 *
 * Surfel of a kept face.  b = (0x3eaaaaab, 0x3eaaaaab, 0x3eaaaaaa) as float32 bits (get_regular_triangle_bary_coords(1)).
 *   mean = (b0 A + b1 B) + b2 C.  colour = the same weights on clamp(image at the three vertices), clamp(x) = 0 if x < 0,
 *   1 if x > 1, else x (a NaN stays).  Axis shifts e^0 = (0xbf3504f3, 0x3f3504f3, 0), e^1 = (0xbed105ec, 0xbed105ec,
 *   0x3f5105ec) as float32 bits: t^j = (e^j_0 A + e^j_1 B) + e^j_2 C, the zero term kept.  first = 0 if |t^0| >= |t^1|,
 *   else 1.  u = t^first, w = the other; w' = w - ((w.u) u) / (u.u) per component; o^first = u, o^other = w'.
 *   scale_j = |o^j * normalized_scales| (the product per component first), scale_2 = normal_scale.
 *   x^j = o^j / floor(|o^j|) per component; n = x^0 x x^1 (each component one product minus the other: n0 = x^0_1 x^1_2 -
 *   x^0_2 x^1_1, n1 = x^0_2 x^1_0 - x^0_0 x^1_2, n2 = x^0_0 x^1_1 - x^0_1 x^1_0); R has the columns (x^0, x^1, n),
 *   m_ij = R[i][j].
 *   Quaternion (w, x, y, z) of R, pytorch3d's matrix_to_quaternion:  sp(t) = sqrt(t) if t > 0 else 0;
 *     q_abs = ( sp(((1 + m00) + m11) + m22), sp(((1 + m00) - m11) - m22), sp(((1 - m00) + m11) - m22),
 *               sp(((1 - m00) - m11) + m22) ).  Candidate rows:
 *       0: ( q_abs0^2, m21 - m12, m02 - m20, m10 - m01 )
 *       1: ( m21 - m12, q_abs1^2, m10 + m01, m02 + m20 )
 *       2: ( m02 - m20, m10 + m01, q_abs2^2, m12 + m21 )
 *       3: ( m10 - m01, m20 + m02, m21 + m12, q_abs3^2 )
 *   k = the first index of the largest q_abs; q = row k / (2 max(q_abs_k, 0.1f)) per component; if q_w < 0 every
 *   component is negated (w >= 0; pytorch3d before the sign was standardised returns q or -q, the same rotation).
 *
 * Two phases.  count: *n_faces (host int; one host synchronisation).  emit, with the same views, maps and workspace, the
 *   workspace untouched in between: means [n_faces,3], scales [n_faces,3], quaternions [n_faces,4], colors [n_faces,3]
 *   float32; nothing is written beyond row n_faces - 1.  No float atomics: every output is a function of the inputs.
 *
 * Voxel pick of indices (g4s_voxel_downsample_emit_index, after g4s_voxel_downsample_count on the n means, same workspace):
 *   per voxel, in float64, s = sum of (double)i / (double)n over the voxel's points in ascending input index, a = s /
 *   count, index = a * (double)n rounded half to even, as int64 -- the arithmetic of voxel_downsample_gaussians, which
 *   recovers an index from open3d's averaged colour.  The index is the rounded mean index of the voxel's points and may
 *   name a surfel of another voxel; the trainer depends on it.  Voxels in ascending (cz, cy, cx) (open3d's order is a hash
 *   map's).
 *
 * Every argument is checked on the host before anything is launched.  The size query is pure host code and returns 0 for
 * arguments out of range.
 */
size_t g4s_chart_surfels_workspace(int n_views, int height, int width);

int g4s_chart_surfels_count(int n_views, int height, int width, int depth_form, const float* const* maps, const float* rays,
                            const unsigned char* const* masks, float ratio_th, int* n_faces, char* workspace,
                            size_t workspace_bytes, void* stream);

int g4s_chart_surfels_emit(int n_views, int height, int width, int depth_form, const float* const* maps, const float* rays,
                           const float* const* images, float normalized_scales, float normal_scale, int n_faces, float* means,
                           float* scales, float* quaternions, float* colors, char* workspace, size_t workspace_bytes,
                           void* stream);

/* index_out [n_voxels] int64. */
int g4s_voxel_downsample_emit_index(int n, int n_voxels, long long* index_out, char* workspace, size_t workspace_bytes,
                                    void* stream);

/* =====================================================================================================================
 * Warp surfels (g4splat_amd/csrc/tsdf/warp_init.hip).
 *
 * The trainer's default first act with --use_downsample_gaussians (2d-gaussian-splatting/train_with_refine_depth.py,
 * "Initialize gaussians", downsample_gaussians_type "warp"; scene/gaussian_model.py
 * get_gaussian_parameters_by_warp_from_depths): one surfel per pixel that no EARLIER view already explains under
 * depth-consistent warping.  tests/warp_init_ref.py restates this section in numpy.  The rules of the Visibility section
 * apply: float32, round-to-nearest-even, correctly rounded / and sqrt, no fused multiply-add, left to right as written.
 * NOT the min / max of that section: every min, max and clamp here propagates a NaN, as torch.min and torch.clamp do
 * (min(a, b) = a if a is a NaN or a < b, else b; max(t, lo) = lo if t < lo, else t).
 *
 * Inputs.  V views in order.  View v has world_view_transform, focal {fx, fy}, a ray record rays[12 v .. 12 v + 11], a depth
 *   map [H_v,W_v] and an image [3,H_v,W_v], all as in the Visibility section; sizes may differ between views.  Scalars:
 *   depth_error_thresh, min_scale, max_scale and the grid g (g <= 0 means 1).  Limit: the lattice cells of all views, the sum
 *   of ceil(H_v / g) ceil(W_v / g), stay below 2^31.
 * Points.  P_v(y,x) is THE back-projection of pixel (y,x) at its depth (g4s_depth_to_points), whatever the depth is: a
 *   non-positive depth still yields a point, and such points are neighbours like any other (the reference's behaviour).
 * Candidates.  Pixel (y,x) of view v is a candidate iff y % g == 0 && x % g == 0 && depth > 0 (a NaN depth is none).
 * Covered.  A candidate p of view i is covered iff for some j < i: with (z, u, v) THE projection of P_i(p) into view j (there
 *   is no second projection), u >= 0 && u <= W_j - 1 && v >= 0 && v <= H_j - 1 && z > 0 -- the borders are closed, which is
 *   not the Visibility section's "in image" --, d = depth_j[rint(v)][rint(u)] with round half to even (torch.round), d > 0,
 *   and SURFACE as written there: |z - d| / (z + 1e-6) < depth_error_thresh.
 * Scale.  dist(a, b) = sqrt((dx*dx + dy*dy) + dz*dz) of the difference.  s = min(min(min(r, l), d), u) * 0.5 over the
 *   distances from P(y,x) to its right, left, lower and upper neighbour point, times float(g) when g > 0.  At a border the
 *   missing neighbour's distance is the opposite one's (the reference's edge replication).  A NaN distance gives a NaN s.
 *   If W_v == 1 or H_v == 1 every s of the view is 1e-3f * 0.5 (times float(g)).
 * Keep.  A pixel is kept iff it is a candidate, is not covered and s < max_scale (a NaN s is dropped).  This is the
 *   reference's final valid_scale_mask folded in; it changes no row and no order.
 * Normal.  n(sy, sx) with sy = clamp(y, 1, H-2), sx = clamp(x, 1, W-2) (the reference's border copy, rows first, then
 *   columns): n = normalize(cross(P(sy+1,sx) - P(sy-1,sx), P(sy,sx+1) - P(sy,sx-1))), cross(a, b) = (a1 b2 - a2 b1,
 *   a2 b0 - a0 b2, a0 b1 - a1 b0), normalize(a) = a / max(sqrt((a0*a0 + a1*a1) + a2*a2), 1e-12f) per component.  If H < 3
 *   or W < 3 the normal is (0, 0, 1).
 * Quaternion (w, x, y, z).  The reference's own construction, not pytorch3d's, without sign standardisation:
 *   z_axis = normalize(n); ref = (0,1,0) if |z_axis_0| > 0.9 else (1,0,0); x_axis = normalize(cross(ref, z_axis)), every
 *   product with a zero of ref kept; y_axis = cross(z_axis, x_axis); the matrix m has the columns (x_axis, y_axis, z_axis).
 *   q = ( sqrt(max(((1 + m00) + m11) + m22, 0)) / 2, sqrt(max(((1 + m00) - m11) - m22, 0)) / 2,
 *         sqrt(max(((1 - m00) + m11) - m22, 0)) / 2, sqrt(max(((1 - m00) - m11) + m22, 0)) / 2 );
 *   q_x *= sign((m21 - m12) + 1e-12f), q_y *= sign((m02 - m20) + 1e-12f), q_z *= sign((m10 - m01) + 1e-12f), sign(t) = 1 if
 *   t > 0, -1 if t < 0, else t (in float32 the 1e-12 only decides the sign of an exact zero);
 *   then q / max(sqrt(((q_w*q_w + q_x*q_x) + q_y*q_y) + q_z*q_z), 1e-12f) per component.
 * Row.  means = P_v(y,x); scales = (max(s, min_scale), max(s, min_scale)); the quaternion; colors = image[:, y, x], unclamped.
 * Order.  Views in order, the kept pixels of a view in row-major order.  No atomics: the same bits from run to run.
 *
 * Two phases.  count writes keep[v], one byte (0 or 1) per lattice cell [ceil(H_v / g), ceil(W_v / g)] -- cell (ly, lx) is
 *   pixel (ly g, lx g) --, and *n_rows (host int; the one host synchronisation of the stage).  emit, with the same views, grid,
 *   keep maps and workspace, the workspace untouched in between, writes means [n_rows,3], scales [n_rows,2], quaternions
 *   [n_rows,4], colors [n_rows,3] float32 and nothing beyond row n_rows - 1.  Depth maps and images are only read.
 *
 * world_view [V,16], focal [V,2], sizes [V,2], rays [V,12] and the pointer arrays are HOST arrays.  Every argument is checked
 * on the host before anything is launched.  The size query is pure host code and returns 0 for arguments out of range.
 */
size_t g4s_warp_init_workspace(int n_views, const int* sizes, int grid);

int g4s_warp_init_count(int n_views, const float* world_view, const float* focal, const int* sizes, const float* const* depth,
                        const float* rays, int grid, float depth_error_thresh, float max_scale, unsigned char* const* keep,
                        int* n_rows, char* workspace, size_t workspace_bytes, void* stream);

int g4s_warp_init_emit(int n_views, const float* world_view, const float* focal, const int* sizes, const float* const* depth,
                       const float* rays, const float* const* images, int grid, float min_scale,
                       const unsigned char* const* keep, int n_rows, float* means, float* scales, float* quaternions,
                       float* colors, char* workspace, size_t workspace_bytes, void* stream);

/* =====================================================================================================================
 * Plane masks (g4splat_amd/csrc/tsdf/plane_masks.hip).
 *
 * What the reference does per view in 2d-gaussian-splatting/planes/plane_excavator.py after the SAM network has run: KMeans
 * over the view's normals, planes/tools.py merge_normal_clusters and remove_small_isolated_areas, the double loop over masks
 * and normal components, the repaint and the mean normal per plane.  The network stays with the caller: its masks are an
 * input.  The pick and merge of clusters, the order of the masks and the numbering of ids run on the host over a few
 * numbers (g4splat_amd/plane_masks.py); this section states what the library computes.  The semantics are the library's own,
 * stated exactly (tests/plane_masks_ref.py restates them in numpy): float32 unless float64 is named, round-to-nearest-even, no
 * fused multiply-add, evaluated left to right as written.  No floating-point atomics; integer atomics only where the result
 * does not depend on the order.  Two runs give the same bits.
 *
 * Views as in "Depth cues": V <= 65535, sizes = {W0, H0, ...}, maps as HOST arrays of V device pointers, pixel q = y W + x.
 *
 * A. k-means (g4s_kmeans_normals).  normals[v] is [H,W,3] float32, k <= G4S_KMEANS_MAX_K, init [V,k,3] (HOST, finite).  A
 *   pixel with a NaN component is invalid: label -1, part of no sum.  Lloyd's algorithm per view, iterations i = 1, 2, ...:
 *   Assignment.  d_j = ((dx dx + dy dy) + dz dz), dx = x - c_j.x and alike, per centre j; the label is the smallest j whose d_j
 *     is below every earlier one (strict <, from d_0): ties go to the smallest index.
 *   Update.  Per cluster the count n_j and the float64 sums of x, y, z of its members in a fixed order: a workgroup owns
 *     G4S_KMEANS_SPAN consecutive pixels, thread t adds pixels t, t + 256, ... of the span in ascending order, a fixed tree
 *     folds the 64 lanes of a wave (lane l += lane l + 32, then 16, ... 1), the four waves are added in order, and lane l of
 *     one wave adds the workgroups' partials l, l + 64, ... in ascending order before the same tree.  new c_j = float32(sum /
 *     n_j); a cluster without members keeps its centre (sklearn relocates it).  shift_j = (ex ex + ey ey) + ez ez in float64,
 *     e = new c_j - c_j.
 *   Stop.  After iteration i >= 2 whose labels all equal those of i - 1: stop, the centres are the new ones, labels stay.
 *     Otherwise if the sum over j in ascending order of shift_j <= tol * ((var_x + var_y) + var_z) / 3, or i = max_iter:
 *     stop, and the pixels are assigned once more with the new centres.  var_x = (Sxx - Sx Sx / n) / n in float64 over the
 *     valid pixels, sums in the fixed order above (the product x x of a float32 is exact in float64).
 *   Outputs: labels[v] int8 [H,W]; centres [V,k,3] float32 and counts [V,k] int32, the members of the final labels (device);
 *     n_iter [V] (HOST) = the last i.  The host waits once per 8 iterations, not once per iteration: a one-wave launch per
 *     iteration writes the view's state, the launches of later iterations return at once for a view that has stopped.
 *
 * B. Opening and components (g4s_normal_components_count / _sizes).  labels[v] int8 [H,W]; lut [V,16] (HOST): label -> rank in
 *   0 .. 15 or -1 (dropped); a label outside 0 .. 15 has rank -1.
 *   Opening (open != 0) with the 9x9 square, all ranks at once.  Pixel p survives the erode iff rank(p) >= 0 and every pixel
 *     of the 9x9 window around p that lies inside the image has rank(p) (pixels outside the image count as members: OpenCV's
 *     default border of an erode).  opened(p) = rank(p) if some pixel of the window around p inside the image survived (pixels
 *     outside count as non-members), else -1.  A survivor in the window of p has p in its own window, so it has p's rank: the
 *     opened masks of the ranks are disjoint.  open == 0: opened = rank.  opened[v], if given, receives it as int8 [H,W].
 *   Components: 8-connectivity among pixels of equal opened rank >= 0.  size = the pixel count.  Components with size >=
 *     min_size[v] (>= 1) are kept and numbered 0 .. n - 1 ascending by (rank, first pixel in raster order); components[v] int32
 *     [H,W] = the number, or -1.  n [V] (HOST) is read back: the one host synchronisation.  g4s_normal_components_sizes, with
 *     the same views and the workspace untouched in between, writes component_sizes[v] int32 [n_v].
 *   This is remove_small_isolated_areas (whose median blur is discarded and whose Otsu threshold of a {0, 255} image is the
 *   identity) followed by the reference's second labelling, which finds the same components again.
 *   Limit: the views have fewer than 2^31 pixels together.
 *
 * C. Join with the masks.  masks[v] is uint8 [M_v,H,W], set iff non-zero (may be NULL for M_v = 0); components[v] as in B
 *   with n_v components (values outside 0 .. n_v - 1 are "none").
 *   g4s_plane_pair_counts: areas [sum M_v] int32 = the set pixels of every mask; pairs [sum M_v n_v] int32, view after view,
 *     pairs[m n_v + c] = the pixels of mask m inside component c.  Both device, cleared and filled.
 *   g4s_plane_paint: order [sum M_v] (HOST) per view a permutation of its masks; pair_ids [sum M_v n_v] (HOST), 0 or an id in
 *     1 .. n_ids[v].  seg[v][p] = pair_ids[m n_v + c] of the LAST mask m of the order with a non-zero id for the pixel's
 *     component c that holds p; 0 if there is none.  id_areas [sum (n_ids[v] + 1)] int32 (device): the pixels per id.
 *   g4s_plane_relabel: relabel [sum (n_ids[v] + 1)] (HOST), relabel[0] = 0, values in 0 .. n_planes[v].  seg[v][p] =
 *     relabel[seg[v][p]] in place.  sums [sum (n_planes[v] + 1), 3] int64 (device): per new id the sum over its pixels of
 *     round-half-even(clamp(x, -2, 2) 2^32) of every normal component x, 0 for a NaN; an integer sum, so independent of the
 *     order (it cannot overflow for fewer than 2^30 pixels).  The caller divides by 2^32 and the area in float64.
 *
 * Differences from the reference, on purpose.  Ids are int32 (the reference's uint8 seg_mask wraps beyond 255 pair ids).
 *   The inputs are never written.  The k-means seeds are the caller's; an empty cluster keeps its centre; the sums are
 *   float64 in a fixed order (sklearn sums float32 in chunks).
 *
 * Every argument is checked on the host before anything is launched.  The size queries are pure host code and return 0 for
 * arguments out of range.
 */
#define G4S_KMEANS_SPAN 4096 /* pixels per workgroup of the k-means sums */
#define G4S_KMEANS_MAX_K 16

size_t g4s_kmeans_normals_workspace(int n_views, const int* sizes);

int g4s_kmeans_normals(int n_views, const int* sizes, const float* const* normals, int k, const float* init, int max_iter,
                       double tol, signed char* const* labels, float* centres, int* counts, int* n_iter, char* workspace,
                       size_t workspace_bytes, void* stream);

size_t g4s_normal_components_workspace(int n_views, const int* sizes);

int g4s_normal_components_count(int n_views, const int* sizes, const signed char* const* labels, const int* lut, int open,
                                const int* min_size, signed char* const* opened, int* const* components, int* n,
                                char* workspace, size_t workspace_bytes, void* stream);

int g4s_normal_components_sizes(int n_views, const int* sizes, const int* n, int* const* component_sizes, char* workspace,
                                size_t workspace_bytes, void* stream);

size_t g4s_plane_pair_counts_workspace(int n_views);

int g4s_plane_pair_counts(int n_views, const int* sizes, const int* const* components, const unsigned char* const* masks,
                          const int* n_masks, const int* n_components, int* areas, int* pairs, char* workspace,
                          size_t workspace_bytes, void* stream);

size_t g4s_plane_paint_workspace(int n_views, int total_masks, int total_pairs);

int g4s_plane_paint(int n_views, const int* sizes, const int* const* components, const unsigned char* const* masks,
                    const int* n_masks, const int* n_components, const int* order, const int* pair_ids, const int* n_ids,
                    int* const* seg, int* id_areas, char* workspace, size_t workspace_bytes, void* stream);

size_t g4s_plane_relabel_workspace(int n_views, int total_ids);

int g4s_plane_relabel(int n_views, const int* sizes, int* const* seg, const float* const* normals, const int* n_ids,
                      const int* relabel, const int* n_planes, long long* sums, char* workspace, size_t workspace_bytes,
                      void* stream);

/* =====================================================================================================================
 * Plane fit (g4splat_amd/csrc/tsdf/plane_fit.hip).
 *
 * What the reference does per global plane id in 2d-gaussian-splatting/planes/refine_depth_with_planes.py between loading its
 * maps and pasting the plane depths: the valid points of every (plane, view) pair, KMeans over their rendered normals, the
 * points of the largest cluster of every pair joined per plane, and RANSACRegressor over a GeneralPlaneRegressor with the
 * mean cluster normal as prior.  The k-means is g4s_kmeans_normals of "Plane masks", unchanged, over [n,1,3] views.  The
 * seeds, the top cluster, the prior, the sample triples and the walk over the inlier counts that picks a trial run on the
 * host over a few numbers (g4splat_amd/plane_fit.py); this section states what the library computes.  The semantics are the
 * library's own, stated exactly (tests/plane_fit_ref.py restates them in numpy): float64 where named, round-to-nearest-even, no
 * fused multiply-add, evaluated left to right as written.  No floating-point atomics; integer atomics only for sums.  Two
 * runs give the same bits.
 *
 * Views as in "Plane masks".  Per view depth [H,W] float32, normals [H,W,3] float32, plane_masks [H,W] int32, conf [H,W]
 * uint8 (set iff non-zero), rays [V,12] (HOST): the Visibility section's ray record.
 *
 * A. Gather (g4s_plane_fit_gather_count / _emit).  Pairs e = 0 .. n_pairs - 1 (at most 65535), pair_view and pair_id (HOST).
 *   Pixel q of the pair's view is valid iff plane_masks[q] == pair_id[e], conf[q] is set, and the three normal components and
 *   the depth are finite.  _count writes pair_count [n_pairs] (HOST), the valid pixels per pair: the one host
 *   synchronisation.  The caller decides which pairs to keep and where: pair_row [n_pairs] (HOST, int64) is a pair's first
 *   output row or -1.  _emit, with the same views and pairs and the workspace untouched in between, writes for every kept
 *   pair, in raster order, points [n_rows,3] = the back-projection of g4s_depth_to_points (the same device function) and
 *   out_normals [n_rows,3] = the normals, both float32.  A pair may be listed several times.  Limit: the views of all pairs
 *   have fewer than 2^31 pixels together.
 *
 * B. Members (g4s_plane_fit_members_count / _emit).  The gathered rows of pair e are pair_offset[e] .. pair_offset[e + 1] - 1
 *   (HOST, from 0 to n_rows); labels [n_rows] int8 (device); top [n_pairs] (HOST).  A row is a member iff its label equals
 *   its pair's top.  Plane p owns pairs plane_pair[p] .. plane_pair[p + 1] - 1 (HOST, from 0 to n_pairs).  _count writes
 *   plane_offset [n_planes + 1] (HOST): the members before each plane, the last entry their number.  _emit, with the
 *   workspace untouched in between, writes plane_points [n_members,3]: the members' points in row order.
 *
 * C. The solver.  Given a centroid c, a covariance C (symmetric 3x3) and optionally a unit prior p with alpha > 0, the
 *   unit normal n that minimises  n^T C n + alpha (1 - |n . p|)^2  -- GeneralPlaneRegressor's objective with the best offset
 *   substituted -- and d = -n . c.  All float64, only + - * / sqrt and comparisons:
 *   A = C, or with a prior A_ij = C_ij + (alpha p_i) p_j (i <= j).  V = I.  G4S_PLANE_FIT_SWEEPS cyclic Jacobi sweeps, each
 *   the rotations (0,1), (0,2), (1,2); a rotation (p,q) with r the third index:
 *     theta = (a_qq - a_pp) / (2 a_pq); tf = 1 / (|theta| + sqrt(theta theta + 1)); t = 0 if a_pq == 0, else -tf if theta < 0,
 *     else tf; c = 1 / sqrt(t t + 1); s = t c; h = t a_pq; a_pp -= h; a_qq += h; a_pq = 0;
 *     (a_rp, a_rq) = (c a_rp - s a_rq, s a_rp + c a_rq); for every row k of V: (v_kp, v_kq) = (c v_kp - s v_kq, s v_kp + c v_kq).
 *   Eigenvalues l_i = a_ii with the columns of V, ordered by the exchanges (0,1), (1,2), (0,1), each made iff the later value is
 *   strictly smaller (ascending, stable); then every column is negated iff its component of largest magnitude (the first of
 *   equals) is negative.
 *   Without a prior y = (1, 0, 0).  With one: b_i = alpha ((v_0i p_0 + v_1i p_1) + v_2i p_2), g_i = l_i - l_0, and with
 *   ratio(b, x) = 0 if b == 0 else b / x: h_i = ratio(b_i, g_i) for i = 1, 2 and hh = h_1 h_1 + h_2 h_2.  The hard case, b_0 == 0
 *   and hh < 1: y = (sqrt(1 - hh), h_1, h_2), the positive root.  Otherwise the root mu of the secular equation sum_i (b_i / (g_i + mu))^2 = 1
 *   is bisected on [0, alpha]: lo = 0, hi = alpha, G4S_PLANE_FIT_BISECTIONS times mid = (lo + hi) 0.5, s = (t_0 t_0 + t_1 t_1) +
 *   t_2 t_2 with t_i = ratio(b_i, g_i + mid) (g_0 + mid = mid), lo = mid if s > 1 else hi = mid; y_i = ratio(b_i, g_i + hi).
 *   n_k = (v_k0 y_0 + v_k1 y_1) + v_k2 y_2, divided by sqrt((n_0 n_0 + n_1 n_1) + n_2 n_2); d = -((n_0 c_0 + n_1 c_1) + n_2 c_2).
 *
 * D. Hypotheses (g4s_plane_fit_hypotheses).  Plane p owns rows plane_offset[p] .. plane_offset[p + 1] - 1 of points (HOST
 *   offsets, at most 65535 planes).  samples [P,T,3] int32 (device) index a plane's own rows; priors [P,3] float64 (HOST) or
 *   NULL.  hypotheses [P,T,4] float64 (device) = (n, d) of C. for the three points x_0, x_1, x_2 promoted to float64: c =
 *   ((x_0 + x_1) + x_2) / 3, e_i = x_i - c, C_jk = ((e_0j e_0k + e_1j e_1k) + e_2j e_2k) / 3.  A triple with an index outside the
 *   plane gives four NaN; nothing is read outside.
 *
 * E. Scoring (g4s_plane_fit_score).  counts [P,T] int32 (device) = the number of the plane's points with
 *   |((x a + y b) + z c) + d| <= threshold in float64, the point promoted.  A NaN is within no threshold.
 *
 * F. Refit (g4s_plane_fit_refit).  best [P] (HOST) = a trial or -1.  inlier_mask [plane_offset[P]] uint8 = the test of E. against the
 *   plane's hypothesis `best` (0 throughout for -1).  moments [P,10] float64 = the sums over the inliers of 1, x, y, z, xx, xy,
 *   xz, yy, yz, zz in the order of "Plane masks" A. (spans of G4S_PLANE_FIT_SUM_SPAN points, thread t adds points t, t + 256,
 *   ..., the tree, the four waves, the fold of the partials by index).  coefficients [P,4] float64 = (n, d) of C. with c_j =
 *   S_j / S_1 and C_jk = S_jk / S_1 - c_j c_k; four NaN for a plane without inliers.
 *
 * Differences from the reference, on purpose.  Pixels with a non-finite normal or depth are dropped (sklearn raises on them).
 *   The solver returns the global minimiser; the reference's SLSQP run from the prior stops up to 5e-5 above it in the
 *   objective and 3.3 degrees away on the 400 cases of tests/test_plane_fit_cpu.py.  Distances are float64 throughout.  Samples and k-means seeds are the caller's.
 *
 * Every argument is checked on the host before anything is launched.  The size queries are pure host code and return 0 for
 * arguments out of range.
 */
#define G4S_PLANE_FIT_SWEEPS 8
#define G4S_PLANE_FIT_BISECTIONS 80
#define G4S_PLANE_FIT_SCORE_SPAN 2048 /* points per workgroup of the scoring kernel */
#define G4S_PLANE_FIT_SUM_SPAN 4096   /* points per workgroup of the refit's sums */

size_t g4s_plane_fit_gather_workspace(int n_views, const int* sizes, int n_pairs, const int* pair_view);

int g4s_plane_fit_gather_count(int n_views, const int* sizes, const float* const* depth, const float* const* normals,
                               const int* const* plane_masks, const unsigned char* const* conf, int n_pairs,
                               const int* pair_view, const int* pair_id, int* pair_count, char* workspace,
                               size_t workspace_bytes, void* stream);

int g4s_plane_fit_gather_emit(int n_views, const int* sizes, const float* rays, const float* const* depth,
                              const float* const* normals, const int* const* plane_masks, const unsigned char* const* conf,
                              int n_pairs, const int* pair_view, const int* pair_id, const int* pair_count,
                              const long long* pair_row, long long n_rows, float* points, float* out_normals, char* workspace,
                              size_t workspace_bytes, void* stream);

size_t g4s_plane_fit_members_workspace(int n_rows, int n_pairs, int n_planes);

int g4s_plane_fit_members_count(int n_rows, int n_pairs, const int* pair_offset, const signed char* labels, const int* top,
                                int n_planes, const int* plane_pair, int* plane_offset, char* workspace, size_t workspace_bytes,
                                void* stream);

int g4s_plane_fit_members_emit(int n_rows, int n_pairs, int n_planes, const float* points, int n_members, float* plane_points,
                               char* workspace, size_t workspace_bytes, void* stream);

/* The workspace of D., E. and F. */
size_t g4s_plane_fit_workspace(int n_planes, const int* plane_offset);

int g4s_plane_fit_hypotheses(int n_planes, const int* plane_offset, const float* points, int n_trials, const int* samples,
                             const double* priors, double alpha, double* hypotheses, char* workspace, size_t workspace_bytes,
                             void* stream);

int g4s_plane_fit_score(int n_planes, const int* plane_offset, const float* points, int n_trials, const double* hypotheses,
                        double threshold, int* counts, char* workspace, size_t workspace_bytes, void* stream);

int g4s_plane_fit_refit(int n_planes, const int* plane_offset, const float* points, int n_trials, const double* hypotheses,
                        const int* best, double threshold, const double* priors, double alpha, unsigned char* inlier_mask,
                        double* moments, double* coefficients, char* workspace, size_t workspace_bytes, void* stream);

/* =====================================================================================================================
 * Mesh rasteriser and dilated depth (g4splat_amd/csrc/tsdf/mesh_render.hip).
 *
 * What the reference asks of pytorch3d: matcha/dm_scene/meshes.py render_mesh_with_pytorch3d (a MeshRasterizer with
 * faces_per_pixel = 1, blur_radius = 0 and a shader over vertex colours) and its one live consumer, get_dilated_depth
 * (2d-gaussian-splatting/extract_mesh_adaptive_tsdf.py:50-137), the `use_dilated_depth` switch of the tetrahedral
 * extraction.  One primitive serves both: a nearest-face-per-pixel z-buffer.  As above, the semantics are this library's
 * own, stated exactly (tests/mesh_render_ref.py restates them in numpy) and NOT bit-equal to pytorch3d: float32,
 * round-to-nearest-even, correctly rounded / and sqrt, no fused multiply-add, evaluated left to right as written; every
 * comparison with a NaN is false; min / max are IEEE minNum / maxNum.
 *
 * Camera.  world_view_transform Wv, projection_matrix Pm (16 HOST floats each, row-major, row-vector @ M: M[r][c] = M[4r + c]),
 *   an image of W x H pixels (W H < 2^31), pixel_offset off = 0.5 or 0.0, znear > 0.
 * Vertices.  For a position p: v_c = ((p0*Wv[0][c] + p1*Wv[1][c]) + p2*Wv[2][c]) + Wv[3][c] for c = 0, 1, 2 and
 *   q_c = ((v_0*Pm[0][c] + v_1*Pm[1][c]) + v_2*Pm[2][c]) + Pm[3][c] for c = 0, 1, 3 (the adaptive-TSDF section's sums);
 *   z = v_2;  sx = ((1 + q_0 / q_3) * float(W)) / 2 - off,  sy = ((1 + q_1 / q_3) * float(H)) / 2 - off, in pixel-index
 *   units: pixel (i, j) = (row, column) samples (sx, sy) = (float(j), float(i)).  off = 0.5 gives the surfel rasteriser's
 *   pixel centres, so a mesh depth map lines up with surf_depth; off = 0 is g4s_atsdf_sample's ix = ((1 + ndc) W) / 2.
 *   A vertex is usable iff z > znear && z < inf && |sx| < inf && |sy| < inf.
 * Faces [F,3] int32, F < 2^31.  A face is skipped, and never used as an address, if it names an index outside [0, V); else
 *   if one of its vertices is not usable ("behind or non-finite", stats[0]; there is no near clipping); else if
 *   |sx| > 32768 or |sy| > 32768 for one of them ("guard band", stats[1]); else if its snapped area is 0.  stats [2] int32
 *   (device, optional) is cleared and counts the two named kinds.  Both windings are drawn.
 * Coverage, in integers.  X_k = rint(sx_k * 256), Y_k = rint(sy_k * 256) (exact inside the guard band);
 *   A = (X_1 - X_0)(Y_2 - Y_0) - (Y_1 - Y_0)(X_2 - X_0), s = sign(A).  For k = 0, 1, 2 with a = (k + 1) mod 3 and
 *   b = (k + 2) mod 3 the oriented edge opposite vertex k is (dx, dy) = s (X_b - X_a, Y_b - Y_a), and at the sample
 *   (PX, PY) = (256 j, 256 i):  E_k = dx (PY - Y_a) - dy (PX - X_a), in 64 bits (below 2^49 inside the face's box).  The
 *   edge owns its samples iff dy < 0 (a left edge: the interior lies towards +x) or dy == 0 && dx > 0 (a top edge: y grows
 *   downwards and the interior lies below).  The sample is covered iff for every k: E_k > 0, or E_k == 0 and edge k owns
 *   its samples.  Two faces that share an edge walk it in opposite directions, so exactly one owns it: a sample inside
 *   the union of the two belongs to exactly one of them, also on the shared edge or on a shared vertex.
 * Weights and depth.  b_k = float(s) * ((sx_b - sx_a) * (float(i) - sy_a) - (sy_b - sy_a) * (float(j) - sx_a)) from the
 *   unsnapped coordinates, negatives replaced by 0; sum = (b_0 + b_1) + b_2; if sum == 0: b_k = float(E_k) and the sum
 *   again.  r_k = (b_k / sum) / z_k;  t = (r_0 + r_1) + r_2;  zpix = 1 / t;  w_k = r_k / t, the perspective-correct weights.
 *   (Weights from the snapped coordinates cost up to 6e-4 of relative depth on sliver faces.)
 * Winner.  Per pixel the covering face of smallest zpix, then of smallest index: the minimum of the 64-bit keys
 *   float_bits(zpix) << 32 | face, by unsigned atomic min over a [H W] buffer of all-ones in the workspace.  Integer min
 *   is order-independent: two runs give the same bits.
 * Resolve, per pixel.  pix_to_face [H,W] int32: the winner or -1.  zbuf [H,W]: the key's high word as float, 0 where
 *   nothing won.  bary [H,W,3]: the winner's w_k, 0 where nothing won.  attr_out [H,W,C], C <= G4S_MESH_RASTER_MAX_CHANNELS:
 *   (w_0 a_0 + w_1 a_1) + w_2 a_2 of attributes [V,C], background [C] (HOST) where nothing won.  normal [H,W,3]: with
 *   u = p_1 - p_0 and v = p_2 - p_0, g = (u_1 v_2 - u_2 v_1, u_2 v_0 - u_0 v_2, u_0 v_1 - u_1 v_0) divided by
 *   len = sqrt((g_0 g_0 + g_1 g_1) + g_2 g_2) -- zero when len is not positive, and where nothing won --; with
 *   G4S_MESH_RASTER_FLIP_NORMALS negated iff ((d_0 g_0 + d_1 g_1) + d_2 g_2) < 0 for d_c = centre_c - ((p_0c + p_1c) + p_2c) / 3
 *   (camera_center, 3 HOST floats); then n_c = (g_0 Wv[0][c] + g_1 Wv[1][c]) + g_2 Wv[2][c]; with
 *   G4S_MESH_RASTER_SURFELS_CONVENTION n_0 and n_1 negated (the reference's two switches, both on by default; the reference
 *   multiplies by sign(d . g), which zeroes the normal of a face seen exactly edge-on).  seen [F] uint8: a plain store of 1
 *   at every winning face, nothing else written: several cameras accumulate into one array.
 *   Every output is optional, but one must be given.
 * Dilated depth (g4s_depth_dilate).  A stack of views of any sizes as in the adaptive-TSDF section: Pm [V,16] (HOST), depth
 *   [H,W] and optionally rgb [3,H,W] per view (all views or none), outputs of the same shapes that share no byte with an input or with
 *   another output (checked on the host).
 *   Everything happens in the view space of the map's own camera, so Wv is not needed.  Per view, with off = 0:
 *   Vertex (i, j): d = depth[i][j], valid iff d > 0 && d < inf;  nx = (2 float(j)) / float(W) - 1, ny = (2 float(i)) / float(H) - 1;
 *   p = (((nx - Pm[2][0]) * d) / Pm[0][0], ((ny - Pm[2][1]) * d) / Pm[1][1], d).
 *   Faces: the grid of get_manifold_meshes_from_pointmaps.  Cell (i, j), i < H - 1, j < W - 1, with a = i W + j has face
 *   i (W - 1) + j = (a, a + W, a + 1) and face (H - 1)(W - 1) + i (W - 1) + j = (a + W + 1, a + 1, a + W): the reference's
 *   indices.  The list is never materialised.  A face with an invalid vertex does not exist: it is neither drawn nor part
 *   of a normal.
 *   Vertex normal: n = 0, then n_c <- n_c + g_c over the incident faces (a, b, c) in ascending face index, g as above with
 *   u = p_b - p_a and v = p_c - p_a; len = max(sqrt((n_0 n_0 + n_1 n_1) + n_2 n_2), 1e-6).  It points towards the camera on
 *   a fronto-parallel patch.
 *   focal = ((Pm[0][0] * float(W)) / 2 + (Pm[1][1] * float(H)) / 2) / 2;  delta = min((dilation_pixels / focal) * d, max_dilation);
 *   p'_c = p_c + delta * (n_c / len).  The grid of the p' is rasterised as above with v = p' (no Wv); colours are
 *   (w_0 a_0 + w_1 a_1) + w_2 a_2 per channel of a = min(max(rgb, 0), 1) at the face's vertices.  Where no face won, the
 *   outputs take the input depth and rgb.
 *   Differences from the reference, on purpose.  One pixel convention on all three sides -- back-projection, raster and the
 *   TSDF's sampler -- where the reference has three, so dilation_pixels = 0 returns the map up to rounding.  The colour is
 *   the interpolated vertex colour (pytorch3d's soft blend adds O(1e-4) of background).  rgb is restored wherever nothing
 *   was drawn (the reference tests the depth for 0 after having filled it, so its rgb fill never fires).  Invalid depths
 *   make holes instead of faces to the origin.  pytorch3d draws no sample that lies exactly on an edge; here the fill
 *   rule is watertight.  The last row and column lie on edges the fill rule leaves out and are served by the fallback.
 *
 * Every argument is checked on the host before anything is launched; sizes beyond the stated limits are refused with a
 * message.  g4s_mesh_raster reads nothing back and does not synchronise -- the list of faces too large for one thread and
 * its length stay on the device --, so it can be captured into a graph.  g4s_depth_dilate uploads its view table like every
 * view-stack entry point (one host synchronisation, before the first launch) and reads nothing back.
 */
#define G4S_MESH_RASTER_MAX_CHANNELS 16
#define G4S_MESH_RASTER_FLIP_NORMALS 1
#define G4S_MESH_RASTER_SURFELS_CONVENTION 2

/* Bytes of device workspace of g4s_mesh_raster (0 for sizes out of range). */
size_t g4s_mesh_raster_workspace(int n_faces, int width, int height);

int g4s_mesh_raster(int n_vertices, const float* vertices, int n_faces, const int* faces, const float* world_view,
                    const float* projection, const float* camera_center, int width, int height, float pixel_offset,
                    float znear, int n_channels, const float* attributes, const float* background, int flags,
                    int* pix_to_face, float* zbuf, float* bary, float* attr_out, float* normal, unsigned char* seen,
                    int* stats, char* workspace, size_t workspace_bytes, void* stream);

/* Bytes of device workspace of g4s_depth_dilate: the view table, 12 B of vertex, 8 B of key and 8 B of list per pixel
 * (0 for sizes out of range: at most 65535 views, fewer than 2^31 pixels together). */
size_t g4s_depth_dilate_workspace(int n_views, const int* sizes);

int g4s_depth_dilate(int n_views, const float* projection, const int* sizes, const float* const* depth,
                     const float* const* rgb, float dilation_pixels, float max_dilation, float znear,
                     float* const* depth_out, float* const* rgb_out, char* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
