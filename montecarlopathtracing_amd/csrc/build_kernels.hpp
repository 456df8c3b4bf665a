// Device build of Morton keys, Morton ordering, leaf records and the implicit tree's boxes (build_kernels.hip).
#pragma once
#include <hip/hip_runtime_api.h>

#include <vector>

#include "../../include/mcpt.h"
#include "device_scene.hpp"
#include "hip_owned.hpp"

namespace mcpt {

struct BuildInputs {            // faces in .obj order, device pointers
    const double* v9;           // [t][9]  v1 v2 v3
    const double* vn9;          // [t][9]
    const double* vt6;          // [t][6]
    const double* nrm3;         // [t][3]  Face::norm
    const int32_t* material;    // [t]
    int t;
    float morton_lo[3], morton_span[3];     // key domain (Scene::morton_lo / morton_span)
};

// fills nodes[Nr] (compact level order), tris[t], shade[t] (leaf order) and d_order[t] (leaf -> .obj face)
hipError_t device_build_reference(const BuildInputs& in, const mcpt_bvh_info& bi, DNode* nodes, DTri* tris, DTriShade* shade,
                                  int32_t* d_order, hipStream_t st);
// The lower part of the fast hierarchy on the device (MCPT_BUILD_DEVICE_FAST): the triangle records sorted by a 63-bit Morton
// code on the scene's bounds [lo, hi] and a complete 4-ary tree over leaves of per_leaf consecutive ones, at most max_levels levels
// high, written as the compressed nodes the walk kernels read.  With t <= 4^(max_levels+1) that is the whole tree (n_top = 1);
// otherwise it is a forest of n_top clusters (nodes 0 .. n_top-1 are their roots, top_boxes their exact boxes, lo[3] hi[3] each)
// for the host to put a SAH tree over (accel_build.cpp: build_fast_upper).  Only ever used to cull (trace_fast.hpp), so its
// shape cannot change a result.  cw and fast_tris receive the buffers built here; the walk needs 3 stack entries per level.
hipError_t device_build_fast(const DTri* leaf_tris, int t, const double lo[3], const double hi[3], int per_leaf, int max_levels, DevBuf<CwNode>& cw, DevBuf<DTri>& fast_tris,
                             int* n_nodes, int* levels, int* n_top, std::vector<double>* top_boxes, double* absmax, hipStream_t st);
// MCPT_BUILD_DEVICE_SAH: the lower part grown on the device by parallel locally-ordered clustering into subtrees of at most max_cluster
// triangles and max_height binary levels, each collapsed into compressed 4-wide nodes (leaves of up to max_leaf triangles where the
// surface-area heuristic, evaluated bottom up with cost_leaf + cost_tri per triangle for a leaf and 1 for a node, prefers a leaf to a split).  Cluster c's
// nodes are a run of *cw starting at top_roots[c] (its root; < 0: the cluster is one leaf and this is its reference); top_boxes as above;
// hipErrorNotSupported: the clusters leave the tree above them too few of the walk's stack entries (take another builder); lower_need = stack entries a walk below a cluster
// root can hold.  rounds = clustering rounds it took.
hipError_t device_build_ploc(const DTri* leaf_tris, int t, const double lo[3], const double hi[3], int max_cluster, int max_height, int radius, int max_leaf,
                             double area_fraction /* of the scene box's area a cluster's box may have; 0: no limit */, double cost_tri, double cost_leaf,
                             int collapse_budget /* stack entries below a cluster root; 0: chosen from the number of clusters */, DevBuf<CwNode>& cw, DevBuf<DTri>& fast_tris, int* n_nodes, int* n_top, std::vector<double>* top_boxes, std::vector<int32_t>* top_roots,
                             int* lower_need, double* absmax, int* rounds, hipStream_t st);
hipError_t device_offset_children(CwNode* nodes, int n, int off, hipStream_t st);     // child >= 0 -> child + off
hipError_t device_gather_tris(const DTri* tris, const int32_t* d_slots, int n, DTri* out, hipStream_t st);
// the pre-test's fp32 record of every slot of the fast triangle array (absmax = largest |coordinate| of the scene)
hipError_t device_build_pre(const DTri* fast_tris, int n, double absmax, DTriPre* out, hipStream_t st);

// ---- geometry updates (update.cpp)
// nrm3[t][3] = Face::norm of the faces v9[t][9], in the loader's operation order
hipError_t device_face_normals(const double* v9, int t, double* nrm3, hipStream_t st);
// out[t][9] = the keyframes v0, v1 blended at time u: (1 - u) * x0 + u * x1 per coordinate, x0 itself where x0 == x1 (three distinct allocations)
hipError_t device_blend_keys(const double* v0, const double* v1, int t, double u, double* out, hipStream_t st);
// tri_faces[i] = .obj face of triangle slot i
hipError_t device_tri_faces(const DTri* fast_tris, int n, int32_t* tri_faces, hipStream_t st);
// leaf_of_face[t] scattered from d_order, then slots[i] = leaf_of_face[tri_faces[i]]: what device_gather_tris refills the slots from
hipError_t device_refit_slots(const int32_t* d_order, int t, const int32_t* tri_faces, int n, int32_t* leaf_of_face, int32_t* slots, hipStream_t st);
// the vetting and the bounds of the vertices v9[t][9] as device creation takes them (synchronises st)
hipError_t device_vet_bounds(const double* v9, int t, bool* coords_ok, double lo[3], double hi[3], hipStream_t st);
// out[n][9] = the vertices of the faces faces[n]
hipError_t device_gather_faces(const double* v9, int t, const int32_t* faces, int n, double* out, hipStream_t st);
// *d_count = number of i with a[i] != b[i]
hipError_t device_count_differing(const int32_t* a, const int32_t* b, int n, int32_t* d_count, hipStream_t st);
// Refit of the hierarchy over the refilled triangle slots: topology kept, every node's planes quantised again around the exact boxes
// below it.  sched = the nodes grouped by depth (level l: sched[level_first[l] .. level_first[l+1])), one launch per level from the
// deepest up; node_box = 6 doubles per node (lo[3], hi[3]), the nodes' own exact boxes.
hipError_t device_refit_levels(CwNode* nodes, int n_nodes, const int32_t* sched, const int* level_first, int n_levels, const DTri* fast_tris, int n_tris, double* node_box,
                               hipStream_t st);
// largest finite |coordinate| of the triangle slots (synchronises st)
hipError_t device_tris_absmax(const DTri* fast_tris, int n, double* absmax, hipStream_t st);
// sum over the non-empty child slots of (area of the stored box) x (1 for a node, triangle count for a leaf) (synchronises st)
hipError_t device_cost_sum(const CwNode* nodes, int n_nodes, double* sum, hipStream_t st);

}  // namespace mcpt
