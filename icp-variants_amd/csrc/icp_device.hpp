// =====================================================================================
// icp_device.hpp -- hand-written HIP kernels of the ICP hot path for gfx950 (MI355X, wave64).
//
// Build contract: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (no fast-math): every fp32
// result is one IEEE rounding per operation, in the operation order of the CPU restatement
// (oracle/icp_oracle.cpp), so match indices / distances / weights are bit-identical to it.
// fp32 sqrt and divide are correctly rounded (hipcc default -fhip-fp32-correctly-rounded-divide-sqrt).
//
// Files: dev_common.hpp, dev_depth.hpp, dev_depth_filter.hpp, dev_knn_brute.hpp, dev_bvh.hpp, dev_normals.hpp, dev_projective.hpp, dev_post.hpp, dev_converge.hpp, dev_solve.hpp,
// dev_fused.hpp, dev_measures.hpp, dev_mesh.hpp, dev_lm.hpp, dev_multi.hpp, dev_gicp.hpp, dev_robust.hpp, dev_colored.hpp, dev_nss.hpp,
// dev_fpfh.hpp, dev_reciprocal.hpp, dev_tsdf_color.hpp, dev_tsdf.hpp, dev_tsdf_mesh.hpp, dev_tsdf_mesh_color.hpp, dev_sdf.hpp, dev_sdf_color.hpp, dev_vgicp.hpp,
// dev_vmap.hpp, dev_hmap.hpp, dev_tsdf_hash.hpp, dev_tsdf_hash_raycast.hpp, dev_tsdf_hash_mesh.hpp, dev_tsdf_hash_evict.hpp, dev_tsdf_hash_color.hpp,
// dev_tsdf_hash_raycast_color.hpp, dev_tsdf_hash_mesh_color.hpp, dev_vmap_prune.hpp, dev_tsdf_cloud.hpp, dev_tsdf_carve.hpp, dev_tsdf_cloud_color.hpp, dev_sdf_cloud.hpp,
// dev_sdf_cloud_color.hpp
// (included below, in this order, inside namespace icpdev).
//
// Kernel map (reference file:line relative to icp-variants/ of the reference):
//   k_deinterleave      AoS -> SoA upload conversion (+ colour features NearestNeighbor.h:212-221)
//   k_knn_brute<DIM>    transformPoints (utils.h:106-118) fused with exact 1-NN, first-minimum argmin
//                       (NearestNeighbor.h:81-97 semantics, squared L2 + squared threshold :181-185);
//                       DIM=6 adds rgb/255 (NearestNeighbor.h:209-303)
//   k_knn_finalize      merges target-split partial results (packed u64 atomicMin) into Match records
//   k_bvh_* / k_knn_bvh exact LBVH index (build once per pair = buildIndex, NearestNeighbor.h:122-141) and its query:
//                       bit-identical argmin to k_knn_brute at O(log M) per query
//   k_projective        NearestNeighborSearchProjective::queryMatches (NearestNeighbor.h:333-421)
//   k_post              transformNormals (utils.h:122-133) + applyWeights (weighting.h:39-99) +
//                       pruneCorrespondences (ICPOptimizer.h:157-174) + validity filter (:594-610) +
//                       normal-equation / moment accumulation (ICPOptimizer.h:676-751, ProcrustesAligner.h:43-55)
//   k_sym_accumulate    second pass of the symmetric objective with the means (ICPOptimizer.h:797-853)
//   k_reduce_solve      fixed-order reduction of block partials + fp64 solve + pose composition
//                       (ICPOptimizer.h:614-620,753-781,855-897; ProcrustesAligner.h:56-66)
//   k_converge_step     stopping on a converged pose (icp_set_convergence_options): the pose increment of an iteration against the
//                       bounds, the streak and the stop word, for the loop forms that launch reduce / solve on their own (dev_converge.hpp)
//   k_rmse_partial      ConvergenceMeasure::rmseAlignmentError (ConvergenceMeasure.h:50-66)
//   k_depth_count /     PointCloud(depthMap, colorFrame, ...) (PointCloud.h:78-165): back-projection, normals, stride and filter of a
//   k_depth_scatter     depth frame as a stable two-pass compaction straight into a context cloud (dev_depth.hpp)
//   k_depth_filter<R>   the bilateral depth filter in front of the trackers (icp_set_depth_filter_options): a tile with its halo and the
//                       two host-built weight tables in LDS, the window of (2R + 1)^2 taps unrolled (dev_depth_filter.hpp)
//   k_*_multi           multi-start ICP (icp_run_multistart): the matcher, post stage and reduce / solve of every start in ONE launch,
//                       start = blockIdx.y; k_score_multi / k_score_fold score the final poses (dev_multi.hpp)
//   k_gicp_normals<K>   Generalized-ICP (plane-to-plane): per-point normals from a K-NN PCA; k_post_gicp weights, rejects and filters as
//   k_post_gicp         k_post does, then adds w^2 J^T M J / w^2 J^T M r of the combined covariance for k_reduce_solve (dev_gicp.hpp)
//   k_robust_*          trimmed ICP and robust kernels: residual keys and their radix histograms, the exact K-th / ceil(K/2)-th smallest
//                       r^2, trimming and IRLS reweighting of the records in place, before the unchanged post kernels (dev_robust.hpp)
//   k_color_gradients<K> colored ICP (Park, Zhou, Koltun 2017): per-point colour gradients of the target from its K nearest neighbours;
//   k_post_colored      k_post_colored weights, rejects and filters as k_post does, then adds the geometric and photometric rows (dev_colored.hpp)
//   k_nss_*             normal-space sampling (Rusinkiewicz and Levoy 2001): buckets of the source normals on a cube map, water-filled
//                       quotas and an exact radix select of each bucket's smallest hashes (dev_nss.hpp)
//   k_fpfh_spfh<K> /    global registration (icp_register_global): FPFH descriptors in two passes, k_feature_match the exact 1-NN in 33
//   k_fpfh              dimensions through LDS tiles, k_ransac_fit / k_ransac_score the three-point hypotheses and their inlier counts (dev_fpfh.hpp)
//   k_reciprocal        reciprocal (mutual nearest-neighbour) rejection: a bounded existence walk over the BVH of the source, one launch per
//                       iteration between the matcher and the post stage (dev_reciprocal.hpp)
//   k_tsdf_integrate /  frame-to-model tracking (icp_track_depth_model): depth frames fused into a truncated signed distance volume, and
//   k_tsdf_raycast      the volume ray-cast from a pose as an organised cloud, to the host or straight into the target (dev_tsdf.hpp)
//   k_tm_*              the zero level set of that volume as an indexed triangle mesh (icp_tsdf_mesh): marching tetrahedra on the Kuhn
//                       triangulation of every cell, as bitmap passes and a stable two-pass compaction (dev_tsdf_mesh.hpp)
//   k_tsdf_*_color /    the coloured model (icp_tsdf_integrate_color, icp_tsdf_raycast_color, icp_tsdf_mesh_color): a second array of running
//   k_tm_colors         colour averages per voxel, fused, ray-cast and meshed with the geometry (dev_tsdf.hpp, dev_tsdf_mesh_color.hpp)
//   k_sdf_accumulate /  direct SDF tracking (icp_tsdf_align_depth, icp_track_depth_sdf): a depth frame's point-to-plane sums read straight
//   k_sdf_solve         from the volume's field and gradient, and the fold, solve and pose update behind them (dev_sdf.hpp)
//   k_sdf_*_color       the same with a photometric row per coloured pixel, read from the colour array in the distance's cell
//                       (icp_tsdf_align_depth_color, icp_track_depth_sdf_color; dev_sdf_color.hpp)
//   k_vg_* /            voxelized GICP (icp_voxelize_target, icp_vgicp_align): the target as a dense grid of cells built from integer sums,
//   k_vgicp_accumulate  and a source point's plane-to-plane sums against the one cell it falls in; k_sdf_solve behind them (dev_vgicp.hpp)
//   k_vmap_insert /     scan-to-map laser tracking (icp_voxel_map_insert, icp_track_scans_vmap): a scan fused at a pose into a persistent grid of
//   k_vmap_records      those cells, and the records of the cells it touched; the alignment is k_vgicp_accumulate's (dev_vmap.hpp)
//   k_hmap_*            the same map stored in a hash table of cells, without an extent (icp_voxel_map_create_hashed): insert, records,
//                       accumulate by probing, growth by rehashing, upload (dev_hmap.hpp)
//   k_htsdf_* /         the TSDF volume stored in 8 x 8 x 8 voxel blocks behind a hash table, without an extent (icp_tsdf_create_hashed): blocks
//   k_hsdf_accumulate   allocated from each depth frame, integrate over the pool, the field by lookup, direct SDF tracking on it (dev_tsdf_hash.hpp)
//   k_htsdf_raycast     the hashed volume seen from a pose (icp_tsdf_raycast_hashed, the target of icp_track_depth_model_hashed): k_tsdf_raycast's
//                       march with every sample's blocks found by lookup, the lowest corner's block first and remembered per lane (dev_tsdf_hash_raycast.hpp)
//   k_htm_*             the zero level set of the hashed volume as a triangle mesh (icp_tsdf_mesh_hashed): k_tm_*'s passes indexed by block rank,
//                       neighbours through a table of ranks, only the mesh crosses to the host (dev_tsdf_hash_mesh.hpp)
//   k_htsdf_evict_* /   streaming the hashed volume (icp_tsdf_evict_blocks, icp_tsdf_insert_blocks): the blocks beyond a radius marked, copied to
//   k_htsdf_present     an outbox and the pool compacted by minimal move; the resident keys among blocks that come back counted (dev_tsdf_hash_evict.hpp)
//   k_htsdf_*_color     the colours of the hashed volume (icp_tsdf_create_color_hashed): a second pool of float4 per voxel by the same pool index --
//                       fusion, upload, the evict's copies, the intensity sample by lookup (dev_tsdf_hash_color.hpp)
//   k_htsdf_raycast_color / the coloured hashed model seen from a pose and meshed (icp_tsdf_raycast_color_hashed, icp_tsdf_mesh_color_hashed): the
//   k_htm_colors        colour of a hit from the blocks its geometry lookup found, a colour per mesh vertex at k_htm_vertices' index
//                       (dev_tsdf_hash_raycast_color.hpp, dev_tsdf_hash_mesh_color.hpp)
//   k_vmap_prune /      forgetting the map's cells beyond a radius of a centre (icp_voxel_map_prune, icp_track_scans_vmap_local), and
//   k_hmap_prune /      the compaction of a hashed table that has vacated slots (dev_vmap_prune.hpp)
//   k_hmap_compact
//   k_*tsdf_*_cloud     a laser scan fused into the TSDF volume, dense or hashed (icp_tsdf_integrate_cloud): the blocks of every ray's band
//                       allocated, the rays' observations summed per voxel in integers, and folded into (tsdf, weight) once (dev_tsdf_cloud.hpp)
//   k_*tsdf_carve_cloud the accumulate of that fuse with free space carved in front of the band (icp_set_tsdf_carve_options): the walk
//                       started earlier, a wave's equal voxels combined before the atomics (dev_tsdf_carve.hpp)
//   k_*tsdf_*_cloud_color the colours of that fuse into a coloured volume (icp_tsdf_integrate_cloud_color): a second walk of the band behind either
//                       accumulate, the points' bytes summed per voxel in integers, and folded into (R, G, B, Wc) once (dev_tsdf_cloud_color.hpp)
//   k_*sdf_accumulate_cloud  direct SDF tracking of a laser scan (icp_tsdf_align_cloud, icp_track_scans_sdf): the resident cloud's point-to-plane
//                       sums read from the volume's field and gradient, dense or hashed; k_sdf_solve behind them (dev_sdf_cloud.hpp)
//   k_*sdf_accumulate_cloud_color  the same for a coloured scan with a photometric row per coloured point (icp_tsdf_align_cloud_color,
//                       icp_track_scans_sdf_photometric): the point's own colour against the intensity field of its cell; k_sdf_solve_color
//                       behind them (dev_sdf_cloud_color.hpp)
//   k_mc_*              vertex clustering of a triangle mesh (icp_mesh_cluster, icp_tsdf_mesh_clustered): the vertices of a grid cell become one,
//                       found through a hash table of cells, equal triangles through a second table; integer sums by rank (dev_mesh_cluster.hpp)
//   k_lm_eval /         CeresICPOptimizer (ICPOptimizer.h:181-483): residuals + Jacobian sums of constraints.h at a point, and the
//   k_lm_step           Levenberg-Marquardt trust-region logic of one ceres::Solve per ICP iteration (dev_lm.hpp)
// =====================================================================================
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <float.h>
#include "../../include/icp_hip.h"

namespace icpdev {

#include "dev_common.hpp"
#include "dev_depth.hpp"
#include "dev_depth_filter.hpp"
#include "dev_knn_brute.hpp"
#include "dev_bvh.hpp"
#include "dev_normals.hpp"
#include "dev_projective.hpp"
#include "dev_post.hpp"
#include "dev_converge.hpp"
#include "dev_solve.hpp"
#include "dev_fused.hpp"
#include "dev_measures.hpp"
#include "dev_mesh.hpp"
#include "dev_lm.hpp"
#include "dev_multi.hpp"
#include "dev_gicp.hpp"
#include "dev_robust.hpp"
#include "dev_colored.hpp"
#include "dev_nss.hpp"
#include "dev_fpfh.hpp"
#include "dev_reciprocal.hpp"
#include "dev_tsdf_color.hpp"
#include "dev_tsdf.hpp"
#include "dev_tsdf_mesh.hpp"
#include "dev_tsdf_mesh_color.hpp"
#include "dev_sdf.hpp"
#include "dev_sdf_color.hpp"
#include "dev_vgicp.hpp"
#include "dev_vmap.hpp"
#include "dev_hmap.hpp"
#include "dev_tsdf_hash.hpp"
#include "dev_tsdf_hash_raycast.hpp"
#include "dev_tsdf_hash_mesh.hpp"
#include "dev_tsdf_hash_evict.hpp"
#include "dev_tsdf_hash_color.hpp"
#include "dev_tsdf_hash_raycast_color.hpp"
#include "dev_tsdf_hash_mesh_color.hpp"
#include "dev_vmap_prune.hpp"
#include "dev_tsdf_cloud.hpp"
#include "dev_tsdf_carve.hpp"
#include "dev_tsdf_cloud_color.hpp"
#include "dev_sdf_cloud.hpp"
#include "dev_sdf_cloud_color.hpp"
#include "dev_mesh_cluster.hpp"

}  // namespace icpdev
