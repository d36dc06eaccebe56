/* scanfuse_internal.h -- NOT part of the drop-in boundary.
 *
 * Entry points libscanfuse.so exports for this repository's own bench.py, tools/ and tests/: measurement aids, scheduling
 * switches, a device self-test and the synthetic stream source.  Nothing a pipeline stage needs is declared here; the
 * product ABI is include/scanfuse.h.  (Round 1 kept these in the public header and read the switches from SF_* environment
 * variables inside sf_fuser_create; they now live behind this header and sf_fuser_tune.)
 */
#ifndef SCANFUSE_INTERNAL_H
#define SCANFUSE_INTERNAL_H

#include "scanfuse.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Scheduling switches of a fuser (results are bit-identical under all of them; tests/test_gpu_tsdf.py runs the matrix):
 *   "batch"       1..32  frames fused per pass over the voxel tiles (default 32: the frame mask of a block is one word; 1 = what sf_fuser_integrate gives a live stream)
 *   "overlap"     0/1    pre-pass / allocation / compaction of the next batch on a second stream (default 1)
 *   "xcd_walk"    0/1    each XCD walks one contiguous eighth of the block list (default 1)
 *   "pipe"        0/1    colourless one-frame passes run the software-pipelined persistent kernel (default 1)
 *   "pipe_overlap" -1/0/1 the next frame's pre-pass / allocation / compaction runs on the second stream beside that kernel: -1 = when the previous
 *                        pass touched more than 512 MiB of tiles (default), 0 never, 1 always
 *   "alloc_group" 1..32  consecutive frames one allocation workgroup walks (default 16: half of a 32-frame pass)
 *   "alloc_ray"   0/1    the allocation kernel's occupancy bitmap in ray space (k_alloc_ray; default: whenever the voxel size lets the window hold a
 *                        pixel tile's rays: >= 2.5 mm voxels with the shipped camera) or as a 32^3-block cube anchored at the first ray (k_alloc)
 *   "tail_wide"   0/1    the LAST pass of a sf_fuser_integrate_batch_device call (no front chain runs beside it) takes the variant of k_integrate that fuses
 *                        the tile in halves at 8 waves per SIMD (default 1: +0.8 % on a 20-frame call; slower for a pass as a whole when allocation runs beside it)
 *   "front_prio"  -1/0/1 which front stream a pass's pre-pass / allocation / compaction goes down: -1 (default) a second one at the device's LOWEST priority beside the
 *                        persistent kernel of one frame per launch out of cache reach (at the highest priority the allocation's 72 KiB workgroups take the LDS the integrate
 *                        kernel's third workgroup per CU needs: 0.54 -> 0.62 of peak HBM shipped at 1 mm), the high-priority one for passes of several frames; 1 always high
 *                        (rounds 2-5), 0 always the second one
 *   "front_lo_lowest" 1/0 that second stream at the device's lowest priority (default) or at the main stream's (0.60-0.61 instead of 0.62).  For a process that ALSO runs
 *                        sf_fuse_run later: the first stream of a priority class opens that class's hardware queues for the life of the process, and sf_fuse_run's seven to
 *                        nine busy streams then run 12 % slower; set 0 there.  Before the stream's first use.
 *   "brick_cache" 0/1    the cube-window allocation kernels (voxels under 2.5 mm, or "alloc_ray" 0) ask the presence cache (one {tag, 64-bit mask} entry per 4x4x4-block brick: "this block is in the table and
 *                        older than this batch") before they probe the hash table (default 1; 0: every look-up probes the table, rounds 1-5).  The allocated
 *                        set and every birth frame are the same either way.
 * Synchronises the fuser.  SF_ERR_INVALID_ARG for an unknown key or a value out of range. */
int sf_fuser_tune(sf_fuser* f, const char* key, int value);

/* How many look-ups of the cube-window allocation kernels went to the hash table since the fuser was created or reset (32-bit, wraps): with the presence cache
 * on, what is left are new blocks, blocks of the previous batch and bricks whose cache entry another brick holds. */
int sf_fuser_alloc_probe_count(sf_fuser* f, uint64_t* out);

/* How many blocks the allocation kernels took to the global hash table one by one because a workgroup's LDS queue / hash set was full (the slow
 * path k_alloc_ray exists to avoid; the volume is the same either way).  tests/test_gpu_tsdf.py asserts 0 on the bench walk's corners. */
int sf_fuser_alloc_direct_count(sf_fuser* f, uint64_t* out);

/* Phases of the most recent sf_fuser_extract_mesh, milliseconds: [0] whole call, [1] live-block list, [2] count pass (k_mc), [3] scan + emit pass,
 * [4] vertex sort (radix sort of the 3T edge keys), [5] heads + scan + weld, [6] triangle sort + gather, [7] downloads (device side), [8] host: output
 * arrays allocated + downloads awaited; then [9] live blocks, [10] triangles, [11] welded vertices.  n <= 12 values are written. */
int sf_fuser_mc_timing(const sf_fuser* f, double* out, int n);

/* One zlib stream through the DEVICE inflate of the frame pipeline (csrc/inflate_gpu.hip): the bytes are sf_zlib_inflate's.  SF_ERR_UNSUPPORTED
 * for streams the device leaves to the host inflater (anything but ONE final fixed-Huffman block -- what the reference's writer and this
 * library's emit; expect_bytes not a multiple of 4), SF_ERR_FORMAT for corrupt streams and streams that inflate to another size. */
int sf_zlib_inflate_gpu(const void* src, uint64_t src_bytes, uint64_t expect_bytes, int device, void* dst);
/* The two kernels of that path timed apart (HIP events) on `count` <= 32 resident streams: microseconds per launch (tools/gpu/inflate_bench.py); skip must be 0 (SF_ERR_UNSUPPORTED otherwise). */
int sf_zlib_inflate_gpu_bench(const void* const* srcs, const uint64_t* src_bytes, int count, uint64_t expect_bytes, int device, int repeats, int skip, double* us_tokens, double* us_copy);

/* Where the frames of the calling thread's last sf_fuse_run were decoded: out[0] zlib depth frames inflated on the device, out[1] by the host threads
 * (streams the device does not take, or SF_INFLATE_HOST), out[2] JPEG colour frames entropy-decoded on the device, out[3] by the host threads. */
int sf_fuse_run_device_counts(uint64_t out[4]);

/* One baseline-JPEG picture through the whole DEVICE path of the frame pipeline: headers parsed and the byte stuffing removed on the host, entropy
 * decoding (csrc/jpeg_huff_gpu.hip) and reconstruction (csrc/jpeg_gpu.hip) on GPU `device`; the bytes are sf_jpeg_decode's.  SF_ERR_UNSUPPORTED
 * for what the device's entropy decoder leaves to the host (restart intervals, sampling factors above 2), SF_ERR_FORMAT for a corrupt stream. */
int sf_jpeg_decode_gpu_huffman(const uint8_t* data, uint64_t bytes, uint32_t width, uint32_t height, int device, uint8_t* dst_rgb);

/* Kernel timing with HIP events on the fuser's stream: when enabled, every integrate launch is bracketed
 * by an event pair; sf_fuser_profile_read sums and clears them (synchronises). */
int sf_fuser_profile_enable(sf_fuser* f, int on);
int sf_fuser_profile_read(sf_fuser* f, double* integrate_ms, uint64_t* launches, uint64_t* blocks);
/* With profiling enabled, sf_fuser_export_dense brackets k_export_dense with an event pair of its own: the microseconds of the calling thread's most
 * recent export (tools/freespace_bench.py); SF_ERR_INVALID_ARG when there was none. */
int sf_fuser_export_dense_kernel_us(float* us);

/* Synthetic stream source (benchmark input): renders frames
 * [first_frame, first_frame+n) of the `total_frames`-frame box-room walk as u16 millimetre depth directly
 * into device memory and returns the n camToWorld poses (n*16 floats, host).
 */
int sf_synth_room_device(void* d_depth, uint64_t frame_stride_bytes, uint64_t first_frame, uint64_t n, uint64_t total_frames,
                         int width, int height, int noise, float* poses_out);
/* The same walk through a box room of room_m = {x, y, z} metres whose corner sits at origin_m (NULL: the world origin): the other scans
 * of SURVEY 8d config 4 (room size +-20 %) and the rooms of config 5's corridor world (one origin per room). */
int sf_synth_scan_device(void* d_depth, uint64_t frame_stride_bytes, uint64_t first_frame, uint64_t n, uint64_t total_frames,
                         int width, int height, int noise, const double room_m[3], const double origin_m[3], float* poses_out);

/* The same with the scene and the noise model chosen ("real-entropy inputs").  noise 0: none; 1: the round-1 LCG ramp (kept
 * for the committed digests); 2: three LSBs hashed per pixel and frame.  scene 0: the empty box room; 1: the room furnished with the 48 boxes of
 * sf_synth_clutter_boxes(room, seed) -- wall furniture, a table island, shelves, lamps -- and, under noise 2, sensor holes (grazing
 * incidence, 0.4 % speckle).  scannet_amd/synth.py renders the same scenes on the host. */
int sf_synth_scene_device(void* d_depth, uint64_t frame_stride_bytes, uint64_t first_frame, uint64_t n, uint64_t total_frames,
                          int width, int height, int noise, int scene, uint32_t seed, const double room_m[3], const double origin_m[3],
                          float* poses_out);
int sf_synth_clutter_boxes(const double room_m[3], uint32_t seed, float* lo_out /* 48 x 3 */, float* hi_out /* 48 x 3 */, int* n_out);

/* Decimation known-answer probe (tests/test_simplify_known_answers.py): of mesh `in` as the quadric edge collapse sees it before the first
 * collapse -- the summed quadric of the edge's end points {a00 a01 a02 a11 a12 a22, b0 b1 b2, c} (error(x) = x'Ax + b'x + c), the position
 * the collapsed vertex would take, the priority of the collapse, and ScaleFactor = 1e8 / diag^6.  Any output may be NULL. */
struct sf_mesh;
int sf_simplify_probe_edge(const struct sf_mesh* in, const sf_simplify_params* p, uint32_t v0, uint32_t v1, double quadric10[10], float position[3],
                           float* priority, double* scale_factor);

/* Stage hooks of the GPU decimation (tests/test_simplify_stages.py; scannet_amd/csrc/simplify_gpu.hip): each call runs ONE part of a round of
 * sf_mesh_simplify_gpu on host arrays -- V vertices, F faces, `alive` one byte per face -- through the helpers its round loop itself calls (same
 * kernels, grids, workgroups, sorts), and returns the result to the host.  Edges are numbered in key order (v0 << 32 | v1, v0 < v1) over the live faces.
 *   edges     k_emit, the sorts, k_vertex_ranges, k_fix_counts, the run-length encode, k_init_quadrics (Q_in == NULL; otherwise Q_in, V x 10 doubles
 *             {a00 a01 a02 a11 a12 a22, b0 b1 b2, c}, is used), k_priority and the quantile.  scale <= 0: ScaleFactor of pos' bounding box.  Arrays
 *             sized for 3 F edges; tau is the clamped threshold of a round that still needs `needed` collapses (`stalled` != 0: no threshold).
 *   winners   the three passes of k_lock / k_winners on priorities of the CALLER's (E_in must be the mesh's edge count): pass_out[e] = the pass in
 *             which edge e won (1..3, 0 = none), taken_out[V] after the third pass, counters = {winners, faces removed, top priority bits}.
 *   collapse  k_collapse on the n edges named (they must be independent, as one round's winners are), x = 3 floats per edge; pos, tri, alive and Q
 *             are updated in place, vdel_out[V] marks the deleted vertices. */
int sf_simplify_stage_edges(int device, uint32_t V, uint32_t F, const float* pos, const uint32_t* tri, const uint8_t* alive, const double* Q_in /*nullable*/,
                            const sf_simplify_params* p, double scale, uint64_t needed, int stalled, uint32_t* E_out, uint64_t* ukey, uint32_t* ucnt,
                            double* Q_out, float* pri, float* x, float* tau_out, double* scale_out /*nullable*/);
int sf_simplify_stage_winners(int device, uint32_t V, uint32_t F, const uint32_t* tri, const uint8_t* alive, uint32_t E_in, const float* pri, float tau,
                              uint32_t round, uint8_t* pass_out, uint8_t* taken_out, uint32_t counters[3]);
int sf_simplify_stage_collapse(int device, uint32_t V, uint32_t F, float* pos, uint32_t* tri, uint8_t* alive, double* Q, uint32_t n, const uint32_t* edges,
                               uint32_t E_in, const float* x, uint8_t* vdel_out);

/* Stage hooks of the GPU mesh clean (tests/test_clean_stages.py; scannet_amd/csrc/clean_gpu.hip): each call runs ONE of the four helpers that
 * sf_mesh_clean_gpu is the composition of, on host arrays -- same kernels, grids, workgroups, sorts and buffers -- and returns its result to the host.
 *   merge       filter 1 on V >= 1 positions: target_out[V] (the vertex each is merged into, itself for a centre), the number of k_settle launches and of
 *               occupied grid cells (both 0 for radius == 0, which takes the sort path), and what k_count_merged counted.  SF_ERR_FORMAT for a
 *               non-finite coordinate and SF_ERR_UNSUPPORTED for more than 2^21 cells on an axis (radius > 0), as the product answers.
 *   faces       k_remap_faces through the CALLER's target[V] (NULL: nobody merged -- the identity is written at the entries the faces name, V may be anything
 *               below 0xFFFFFFF0 and no positions are needed), the select, the duplicate sorts and k_dup_flags, the second select: verdict_out[F] = 0 kept,
 *               1 degenerate, 2 duplicate; tri_out = the F - degenerate - duplicate surviving triples (target applied) in order
 *   components  k_edge_keys, the sort, k_link, k_roots, k_component_flags on F faces: root_out[F], size_out[F] (the component's size AT its root, 0
 *               elsewhere), keep_out[F], counters = {components, components below min_faces, faces in them}
 *   compact     k_mark_used, the scan, k_gather_vertices, k_remap_tris: used_out[V] (0 / 1), remap_out[V] (the exclusive scan: used vertices below v),
 *               the *vertices_out gathered positions and colours (col NULL: none) and the F remapped triples (F may be 0)
 * sf_clean_probe_merge: the host filter's clustering alone (clean.cpp's merge_close), target_out[V]. */
int sf_clean_stage_merge(int device, uint32_t V, const float* pos, float radius, uint32_t* target_out, uint32_t* launches_out, uint32_t* cells_out,
                         uint32_t* merged_out);
int sf_clean_stage_faces(int device, uint32_t V, uint32_t F, const uint32_t* tri, const uint32_t* target /*nullable*/, uint8_t* verdict_out, uint32_t* tri_out,
                         uint32_t* degenerate_out, uint32_t* duplicate_out);
int sf_clean_stage_components(int device, uint32_t F, const uint32_t* tri, uint32_t min_faces, uint32_t* root_out, uint32_t* size_out, uint8_t* keep_out,
                              uint32_t counters[3]);
int sf_clean_stage_compact(int device, uint32_t V, uint32_t F, const float* pos, const uint8_t* col /*nullable*/, const uint32_t* tri, uint32_t* used_out,
                           uint32_t* remap_out, float* pos_out, uint8_t* col_out, uint32_t* tri_out, uint32_t* vertices_out);
int sf_clean_probe_merge(uint32_t V, const float* pos, float radius, uint32_t* target_out);

/* Device self-test: the hand-expanded correctly rounded divisions of the integrate and allocation kernels against the hardware's IEEE
 * division -- all 2^23 mantissas x 9 exponents for 1/x, 511 integer divisors x 2^21 numerators for n/m, 2^28 general operand pairs
 * (incl. near-exact and near-half-way quotients) for a/b.  All three counts must be 0 (tests/test_gpu_tsdf.py). */
int sf_selftest_division(int device, uint64_t* recip_mismatches, uint64_t* quot_mismatches, uint64_t* div_mismatches);
/* Device self-test: 1 / b by ONE Newton step from the hardware's reciprocal seed, for every one of the 2^32 bit patterns as b; every normal b whose
 * correctly rounded reciprocal is normal is compared with 1.0f / b.  *mismatches = how many differ; patterns_out[0 .. min(*mismatches, capacity)) = bit
 * patterns of b that do (which ones, when there are more than `capacity`, is up to the scheduling; capacity 0: none).  *shipped (may be NULL) = 1 when
 * the kernels' reciprocal (recip_rn, fuser_internal.h) IS that one step, 0 when it takes two.  A few milliseconds. */
int sf_selftest_recip_one_step(int device, uint64_t* mismatches, uint32_t* patterns_out, uint32_t capacity, int* shipped);
/* Device self-test: the 256 per-weight records of the multi-frame integrate kernels' LDS table, built on the device by the function the kernels
 * call.  out[4 w .. 4 w + 3] = bits of (float)w, of (float)(w + 1), of 1.0f / (float)(w + 1), and min(w + 1, 255) << 24 | (w == 0 ? 0x00FFFFFF : 0). */
int sf_selftest_weight_records(int device, uint32_t* out /* 256 x 4 */);

/* Measurement aid (bench.py roofline_single_frame.pattern_ceiling): the memory traffic of the most recent integrate pass
 * without its arithmetic -- every tile of that pass's list is read and (read_only == 0) written back unchanged, with the
 * integrate kernel's launch geometry; iters timed launches, average duration in microseconds.  The volume is unchanged. */
int sf_fuser_calib_tile_rmw(sf_fuser* f, int read_only, int iters, double* avg_us, uint32_t* tiles);
/* The same traffic taken apart (bench.py roofline.hbm_out_of_cache.rmw_decomposition).  mode bit 0: read only; bit 1: tiles 0 .. n - 1 of the pool -- one
 * contiguous span of the same size -- instead of the pass's scattered list; bits 2-3: log2 of the tiles a wave reads before it writes them back (1 / 2 / 4).
 * Every tile is written back as read: the volume is unchanged. */
int sf_fuser_calib_tile_rmw_ex(sf_fuser* f, int mode, int iters, double* avg_us, uint32_t* tiles);

/* Test hook of the camera tracker (tests/test_track.py): one level's 29-value system for the estimate T and the reference pose T_ref (DESIGN.md
 * "Camera tracking": the 21 entries of J^T J, row by row of its upper triangle, the 6 of J^T r, sum r^2, the count), summed as sf_fuser_track sums
 * it.  depth: host u16 at the input size.  mask (optional): the level's W_l x H_l image, 1 where a pixel is a correspondence. */
int sf_fuser_track_system(sf_fuser* f, const uint16_t* depth, int level, const float T[16], const float T_ref[16], const sf_track_params* t,
                          double sys[29], uint8_t* mask);

/* Its twin with the colour term (tests/test_track_colour.py): the level's 31-value system as sf_fuser_track_rgbd sums it -- the 27
 * weighted sums, the depth term's sum r^2 and count, the colour term's sum r_c^2 and count.  rgb: the host picture (NULL: colour_weight must be 0). */
int sf_fuser_track_rgbd_system(sf_fuser* f, const uint16_t* depth, const uint8_t* rgb, int level, const float T[16], const float T_ref[16],
                               const sf_track_params* t, double sys[31], uint8_t* mask);

/* Test hook of the global alignment (tests/test_align.py), the twin of sf_fuser_track_system: the P per-pair 29-value systems at the given poses
 * (DESIGN.md section 4e), summed as sf_fuser_align sums them, without solving.  depth: K host frames, u16 at the input size; sys: P x 29 doubles. */
int sf_fuser_align_system(sf_fuser* f, const uint16_t* depth, uint64_t K, const float* poses, const int32_t* pairs, uint64_t P, const sf_align_params* a,
                          double* sys);
/* Its twin with the colour term (tests/test_align_colour.py): the P per-pair 31-value systems as sf_fuser_align_rgbd sums them --
 * the 27 weighted sums, the depth term's sum r^2 and count, the colour term's sum r_c^2 and count.  rgb: K host pictures (NULL: colour_weight must be 0);
 * sys: P x 31 doubles. */
int sf_fuser_align_rgbd_system(sf_fuser* f, const uint16_t* depth, const uint8_t* rgb, uint64_t K, const float* poses, const int32_t* pairs, uint64_t P,
                               const sf_align_params* a, double* sys);

/* Stage hook of the batched group solve (tests/test_align_scan.py; scannet_amd/csrc/align_scan.hip): k_group_solve ALONE on GPU `device`, on
 * caller-supplied per-pair systems.  Group g has n = group_first[g + 1] - group_first[g] members (1..16) and the pairs pair_first[g] ..
 * pair_first[g + 1] - 1 (at most 240) of local_pairs (2 x P int32: source, target as member indices 0..n-1); valid_masks[g] bit k: member k takes part;
 * sys: P x nsys doubles (nsys 29 or 31).  Out, per group: xi (6 doubles per member slot, M x 6 in all), status, pairs used, the connected flags (bit k)
 * and the four sums {counts, r^2, colour counts, colour r^2}. */
int sf_align_group_solve_stage(int device, uint64_t G, const int32_t* group_first, const int32_t* pair_first, const int32_t* local_pairs,
                               const uint32_t* valid_masks, const double* sys, int nsys, int min_pair_correspondences, double* xi_out, int32_t* status_out,
                               int32_t* used_out, uint32_t* conn_out, double* sums_out);

/* Stage hooks of the 2-D annotation filter (tests/test_filter2d_stages.py; scannet_amd/csrc/filter2d.hip): each call runs ONE kernel of the filter on host
 * arrays on GPU `device`, through the launcher sf_filter2d_frame uses for it (same grid, same workgroup, same dynamic LDS), and returns the output to the
 * host.  Images are row-major, w x h.  Sides are 1 .. 16384 (2 .. 16384 for the resamples, whose scale divides by side - 1).
 * Window radius: at most 35 -- what k_f2d_vote's dynamic-LDS budget holds (the 80 x 256 x 4 B histogram + (2r + 1)^2 x 4 B spatial table <= 100 KiB;
 * r = 36 would need 103 236 B); the bilateral hook takes the same bound on its radius ceil(2 sigma_d), i.e. sigma_d <= 17.5.  Anything else is
 * SF_ERR_INVALID_ARG, not a launch.
 *   prepare          depth16[dn] (mm) -> depth_out[dn] (m, 0 -> -inf), rgb[3 cn] -> intensity_out[cn]
 *   bilateral        in -> out, radius ceil(2 sigma_d)
 *   resample_float / resample_uchar
 *                    `out` (ow x oh) is BOTH the initial contents of the output and the result: pixels whose source position rounds outside keep it
 *   vote             one pass of the weighted vote over a (2 radius + 1)^2 window
 *   to_label         label_out[i] = instance_to_label[instance[i]] */
int sf_filter2d_stage_prepare(int device, const uint16_t* depth16, int dn, const uint8_t* rgb, int cn, float* depth_out, float* intensity_out);
int sf_filter2d_stage_bilateral(int device, const float* in, float sigma_d, float sigma_r, int w, int h, float* out);
int sf_filter2d_stage_resample_float(int device, const float* in, int iw, int ih, float* out, int ow, int oh);
int sf_filter2d_stage_resample_uchar(int device, const uint8_t* in, int iw, int ih, uint8_t* out, int ow, int oh);
int sf_filter2d_stage_vote(int device, const uint8_t* instance_in, const float* depth, const float* intensity, const uint8_t instance_to_idx[256],
                           const uint8_t idx_to_instance[80], int radius, int w, int h, float sigma_d, float sigma_r, float intensity_scale,
                           uint8_t* instance_out);
int sf_filter2d_stage_to_label(int device, const uint8_t* instance, const uint16_t instance_to_label[256], int n, uint16_t* label_out);
/* Element-wise probe of the filter's two Gaussians as the kernels evaluate them (exp table in LDS; the range Gaussian through its three-operation
 * quotient): out_r[i] = gaussR(sigma, dist[i]), out_d[i] = gaussD(sigma, dx[i], dy[i]).  Either group (dist + out_r, or dx + dy + out_d) may be NULL.
 * dist[i]^2 must be finite in binary32 (|dist| < 1.8e19): the pipeline forms no distance above 65.535 (metres of depth) or 10 (scaled intensity), and
 * the quotient scheme is not defined for an infinite dividend. */
int sf_filter2d_selftest_gauss(int device, float sigma, const float* dist, const int32_t* dx, const int32_t* dy, uint64_t n, float* out_r, float* out_d);

/* Stage hooks of the axis alignment (tests/test_alignment.py, tests/test_alignment_gpu.py): each call runs ONE stage of
 * sf_axis_align_estimate on host arrays -- on the host for device = -1, else the stage's kernels alone on that GPU (scannet_amd/csrc/axis_align.hip) --
 * and returns its output to the host.  xyz / normals: 3 floats per vertex; tris: 3 u32 per face, every index below num_vertices.
 *   normals    vertex normals (k_aa_normals)
 *   planes     the clustering (k_aa_match + k_aa_commit per batch), the stable sort by size and removeSmallClusters: index_out[v] = the cluster of vertex
 *              v in creation order; *n_founded clusters in all; the *n_sorted <= capacity clusters of at least p->min_cluster_points points, largest
 *              first: ids (creation order), table (10 floats each: representative normal, d, sumNormal, sumPoint), counts, and behind[] = the vertices
 *              further than p->behind_dist behind each (k_aa_behind); counters = {batches, dirty re-evaluations, fallback rescans} (0 on the host)
 *   behind     k_aa_behind alone on K representative planes (4 floats each)
 *   cov        the blocked double sums of the members of `cluster` within inlier_dist of the plane rep4 (k_aa_cov): {n, x, y, z, xx, xy, xz, yy, yz, zz}
 *   transform  positions through a row-major 4x4 with the bounding box {min x y z, max x y z} of the result (k_aa_transform); xyz_out may be NULL
 *   tune       "batch": vertices per speculation batch, 64..1024 in steps of 64 (default 1024), for the calls of this process that follow;
 *              "profile" 0 / 1: the device clustering brackets every launch with HIP events and fills gpu_seconds_match / _commit (default 0) */
/*   up         the up vector of a trajectory (host only): up3, *source (0 views, 1 gravity), *no_gravity = frames whose closest record had none */
int sf_axis_align_stage_up(const struct sf_sens* sens, uint32_t gravity_min_records, float up3[3], int32_t* source, uint64_t* no_gravity);
int sf_axis_align_stage_normals(const float* xyz, uint64_t num_vertices, const uint32_t* tris, uint64_t num_faces, int device, float* normals_out);
int sf_axis_align_stage_planes(const float* xyz, const float* normals, uint64_t num_vertices, const sf_axis_align_params* p, int device, uint32_t* index_out,
                               uint64_t* n_founded, uint32_t* ids, float* table10, uint32_t* counts, uint32_t* behind, uint64_t capacity, uint64_t* n_sorted,
                               uint64_t counters[3]);
int sf_axis_align_stage_behind(const float* xyz, uint64_t num_vertices, const float* reps4, uint64_t K, float behind_dist, int device, uint32_t* counts_out);
int sf_axis_align_stage_cov(const float* xyz, const uint32_t* index, uint64_t num_vertices, uint32_t cluster, const float rep4[4], float inlier_dist, int device,
                            double sums10[10]);
int sf_axis_align_stage_transform(const float* xyz, uint64_t num_vertices, const float m[16], int device, float* xyz_out, float bbox6[6]);
int sf_axis_align_tune(const char* key, int value);

/* Stage hooks of the annotation projector (tests/test_project_stages.py; scannet_amd/csrc/project.hip): each call runs ONE launch group of
 * sf_projector_run on an existing projector -- through the helper sf_projector_run itself launches it with (same kernels, same grids, same stream) --
 * on host arrays, and returns the output to the host.  n = 1 .. sf_projector_max_batch() frames; images are row-major, color_w x color_h per frame.
 *   raster    k_pa_vertex + k_pa_raster + k_pa_raster_big for n poses (cam2world as for sf_projector_run): keys_out = the raw depth buffer,
 *             {z_ndc bits << 32 | triangle index} per pixel, all-ones where nothing was drawn (and everywhere in a frame without a valid pose);
 *             late_counts_out[n] = how many (triangle, half) entries k_pa_raster queued for k_pa_raster_big in each frame
 *   resolve   k_pa_resolve alone on the caller's keys (every index below the mesh's triangle count, else SF_ERR_INVALID_ARG and no launch);
 *             orig_depth n x depth_w*depth_h or NULL (no depth-consistency filter); outputs = the images BEFORE the vote; zcam_out may be NULL
 *   vote      k_pa_vote alone (needs no mesh) */
int sf_projector_stage_raster(sf_projector* p, int n, const float* cam2world, uint64_t* keys_out, uint32_t* late_counts_out);
int sf_projector_stage_resolve(sf_projector* p, int n, const uint64_t* keys_in, const uint16_t* orig_depth, uint8_t* instance_out, uint16_t* label_out,
                               float* zcam_out);
int sf_projector_stage_vote(sf_projector* p, int n, const uint8_t* instance_in, const uint16_t* label_in, uint8_t* instance_out, uint16_t* label_out);

/* Stage hooks of the calibrate stage (tests/test_calibrate_stages.py; scannet_amd/csrc/calibrate.hip): each call runs ONE of the four launches of
 * sf_calibrator_run_device on an existing calibrator -- through the helper sf_calibrator_run_device itself launches it with (same kernel, grid, workgroup
 * and stream) -- on host arrays of n = 1 .. sf_calibrator_max_batch() contiguous frames, and returns the output to the host.  The sizes must be the
 * calibrator's (w x h depth, cw x ch colour); anything else, or n out of range, is SF_ERR_INVALID_ARG and no launch.
 *   undistort_rgb  k_undistort_rgb; the frames sit in the staging buffers of sf_calibrator_run, frame j at j * cw*ch*3 bytes
 *   prepare        k_depth_prepare on raw u16 frames: und_out = the undistorted, table-corrected depth in metres; vert_out = 4 floats per pixel, the
 *                  mesh vertex {target x, target y, projected z, valid (1 / 0)}; zbuf_out = the cleared depth buffer (the bits of 1.0f)
 *   raster         k_raster_quads on the caller's depth in metres, vertex records and INITIAL depth buffer; zbuf_out = the buffer as raw 32-bit words.
 *                  The depth test orders bit patterns: the initial buffer must lie in [0, 1] and a valid vertex must not carry a negative z (what
 *                  k_depth_prepare guarantees), else SF_ERR_INVALID_ARG
 *   finalize       k_finalize on the caller's depth buffer and undistorted colour frames (rgb NULL: nothing is invalidated; cw, ch are then ignored) */
int sf_calibrator_stage_undistort_rgb(sf_calibrator* c, int n, int cw, int ch, const uint8_t* rgb_in, uint8_t* rgb_out);
int sf_calibrator_stage_prepare(sf_calibrator* c, int n, int w, int h, const uint16_t* depth_in, float* und_out, float* vert_out, uint32_t* zbuf_out);
int sf_calibrator_stage_raster(sf_calibrator* c, int n, int w, int h, const float* und, const float* vert, const uint32_t* zbuf_in, uint32_t* zbuf_out);
int sf_calibrator_stage_finalize(sf_calibrator* c, int n, int w, int h, int cw, int ch, const uint32_t* zbuf, const uint8_t* rgb, uint16_t* depth_out);

/* Stage hooks of the mesh render (tests/test_render.py, tests/test_render_gpu.py).
 *   nodes      the tree of the renderer's mesh as the traversal reads it: boxes6 = {min x y z, max x y z} per node (padded as stored), links2 =
 *              {skip, info} per node (info & 15: the leaf's triangle count, 0 for an inner node); either may be NULL; *n_nodes always comes back,
 *              SF_ERR_BOUNDS when capacity (in nodes) is smaller
 *   rays       closest hit of n rays {origin x y z, direction x y z} (finite; the direction as given, not normalised) on the renderer's device
 *              (k_render_rays) or on the host: tri_out = the mesh index of the triangle or 0xFFFFFFFF, tuv_out = {t, u, v} (0 on a miss)
 *   sample     the bounce direction about unit normal n3 for (pixel, sample, bounce) (host)
 *   tune       "leaf": the most triangles the builder leaves in a leaf, 1..15 (default 4), for the sf_renderer_set_mesh calls that follow */
int sf_render_stage_nodes(const sf_renderer* r, float* boxes6, uint32_t* links2, uint64_t capacity, uint64_t* n_nodes);
int sf_render_stage_rays(sf_renderer* r, uint64_t n, const float* rays6, uint32_t* tri_out, float* tuv_out);
int sf_render_stage_sample(const float n3[3], uint32_t pixel, uint32_t sample, uint32_t bounce, float dir3[3]);
int sf_render_tune(const char* key, int value);

/* The raw sums of a depth-distortion table estimator (tests/test_depth_lut.py, tests/test_depth_lut_gpu.py): acc and div,
 * (width / 2) x (height / 2) x n_slices floats each, before the division; images / used (nullable) = how many were added / passed the angle filter. */
int sf_lut_estimator_sums(sf_lut_estimator* e, float* acc, float* div, uint64_t* images, uint64_t* used);

/* Stage hooks of the fusion front chain (tests/test_front_stages.py; scannet_amd/csrc/fuser_prepass.hip, fuser_alloc.hip, fuser_compact.hip, fuser_blocks.hip;
 * DESIGN.md section 3): each call runs ONE stage of a pass on an existing fuser through the launcher run_batch itself uses for it (sf_launch_prepass,
 * sf_launch_alloc, sf_launch_compact, sf_compact_live: the same choice of kernel, grid and workgroup, the buffers of batch slot 0), on the fuser's main
 * stream, with both streams drained before and after.  n = 1..32 frames; depth = n host frames of the fuser's INPUT size, poses = n x 16 floats.  Every
 * argument is checked before anything is launched: anything else is SF_ERR_INVALID_ARG and no launch.
 *   prepass  k_prepass.  Colour is none, OR rgb (n tight RGB8 pictures at the colour size, or the integration size where the fuser has none; the device copy
 *            is placed `misalign` = 0..7 bytes past an aligned address), OR jpeg (one baseline stream per frame, taken through the library's own
 *            jpeg_decode_coef -> jpeg_gpu_planes, the planes and layout handed to the kernel as sf_fuse_run hands them; what that path leaves to the host
 *            decoder is SF_ERR_UNSUPPORTED).  depthf_out: n x W*H floats; texel_out (with colour, else NULL): n x W*H texels {depth bits | rgb << 32}
 *   alloc    the front chain up to and including the allocation as ONE pass: seq0 = the fuser's next sequence number, which advances by n.  head: the
 *            pass is the first of a multi-pass call (groups of at most 4 frames).  fuse_pre 1: k_alloc_ray converts the depth itself -- an error unless
 *            run_batch would pick that variant (one frame, ray-space window, no resampling).  depthf_out (nullable): the float depth the pass wrote.
 *            deltas = what the pass added to {blocks taken to the table one by one, look-ups that went to the table, failures}
 *   compact  sf_launch_compact alone on the present directory for n poses and an explicit seq0: the list (directory slots; order is scheduling, ascending
 *            within a workgroup's stretch), the masks, the 64-bit counter word (list length | last frame's count << 32) and what the launch added to
 *            {sum of the per-frame counts, sum of the list lengths}.  capacity (entries of list_out / mask_out) must hold the directory's used stretch.
 *            n == 1 reads no birth stamp: a one-frame pass only meets blocks born by its own frame or earlier
 *   live     sf_compact_live: every live block (include_ghosts 1) or every live block this fuser owns (0)
 *   dump     host copies of the whole table (key, ptr, birth: total slots each), the heap, block_keys, block_entry, block_flags (num_sdf_blocks each) and the
 *            48 counter words */
int sf_fuser_stage_prepass(sf_fuser* f, int n, const uint16_t* depth, const uint8_t* rgb /*nullable*/, int misalign, const uint8_t* const* jpeg /*nullable*/,
                           const uint64_t* jpeg_bytes, float* depthf_out, uint64_t* texel_out /*nullable*/);
int sf_fuser_stage_alloc(sf_fuser* f, int n, const uint16_t* depth, const float* poses, int head, int fuse_pre, float* depthf_out /*nullable*/, uint64_t deltas[3]);
int sf_fuser_stage_compact(sf_fuser* f, int n, const float* poses, uint32_t seq0, int32_t* list_out, uint32_t* mask_out, uint64_t capacity, uint64_t* counter_word,
                           uint64_t deltas[2]);
int sf_fuser_stage_live(sf_fuser* f, int include_ghosts, int32_t* list_out, uint64_t capacity, uint64_t* n_out);
int sf_fuser_stage_dump(sf_fuser* f, uint64_t* key_out, int32_t* ptr_out, uint32_t* birth_out, int32_t* heap_out, uint64_t* block_keys_out, int32_t* block_entry_out,
                        uint8_t* block_flags_out, int32_t* counters_out);

/* The bin stage of the nearest-face search alone (tests/test_voxel_labels_gpu.py; scannet_amd/csrc/voxel_labels.hip): on a device
 * k_vl_count, k_vl_scan and k_vl_fill as sf_voxlabel_nearest_faces launches them, on the host (device = -1) the host path's bins.  counts / offsets: one
 * per tile of 8^3 nodes, x fastest; list: *total face indices, tile after tile (the order within a tile is free); SF_ERR_BOUNDS when capacity is short.
 * Any output may be NULL. */
int sf_voxlabel_stage_bins(const sf_grid_header* h, const float* xyz, uint64_t num_vertices, const uint32_t* tris, uint64_t num_faces, float band, int device,
                           uint32_t* counts, uint32_t* offsets, int32_t* list, uint64_t capacity, uint64_t* total);

/* Device microseconds (HIP events) of the most recent device call of this process: the bin stage (k_vl_count, k_vl_scan, k_vl_fill), the search
 * (k_vl_clear, k_vl_nearest), and k_vl_sample (tools/voxel_labels_bench.py).  Any pointer may be NULL. */
int sf_voxlabel_kernel_us(float* bins_us, float* nearest_us, float* sample_us);

/* The key, scan and fill stage of the object voxeliser alone (tests/test_object_voxels_gpu.py; scannet_amd/csrc/object_voxels.hip, DESIGN.md section
 * 4n): on a device k_ov_key, k_ov_scan and k_ov_fill as sf_objvox_voxelize launches them, on the host (device = -1) the host path's grouping.
 * face_object: one per face, 0 where the face has no object or is not counted; counts / offsets: num_objects + 1 entries, indexed by the
 * vertex_object value (entry 0 holds nothing); list: the faces, object after object, in no particular order within one.  list may be NULL (then
 * capacity is not read); *total = entries in all.  Any output may be NULL. */
int sf_objvox_stage_faces(const float* xyz, uint64_t num_vertices, const uint32_t* tris, uint64_t num_faces, const uint32_t* vertex_object, uint32_t num_objects,
                          int device, uint32_t* face_object, uint32_t* counts, uint32_t* offsets, uint32_t* list, uint64_t capacity, uint64_t* total);

/* Device microseconds (HIP events) of the most recent device call of this process: grouping and cubes (k_ov_key .. k_ov_box), k_ov_raster, k_ov_emit
 * (tools/object_voxels_bench.py).  Any pointer may be NULL. */
int sf_objvox_kernel_us(float* group_us, float* raster_us, float* emit_us);

/* The SF_EVAL_AP_OVERLAPS overlap thresholds sf_eval_ap_finish compares against, bit for bit (tests/test_evaluation.py holds them against numpy's). */
int sf_eval_ap_thresholds(double* thresholds);

/* PMC calibration stream (tools/pmc_calibrate.py): known-byte-count 16 B/lane RMW + read-only launches. */
int sf_calib_stream(int device, uint64_t bytes, int iters);

#ifdef __cplusplus
}
#endif
#endif
