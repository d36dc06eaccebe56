// axis_align_internal.h -- the stages of the axis alignment as one interface with two implementations: the host loops (axis_align.cpp) and the
// kernels (axis_align.hip).  The driver of the rule (axis_align.cpp) and the stage hooks of scanfuse_internal.h talk to either through it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "axis_align_math.h"
#include "common.h"

namespace sf {
namespace aa {

struct Ops {   // a working set: positions, faces, normals and the per-vertex cluster index stay where the implementation keeps them
  virtual ~Ops() {}
  double split[2] = {0.0, 0.0};   // device path under profile(): seconds in k_aa_match and in k_aa_commit of the last cluster()
  virtual int set_positions(const float* xyz, size_t nv) = 0;
  virtual int set_faces(const uint32_t* tri, size_t nf) = 0;
  virtual int set_normals(const float* n) = 0;
  virtual int set_index(const uint32_t* idx) = 0;
  virtual int get_positions(float* xyz) = 0;
  virtual int get_normals(float* n) = 0;
  virtual int get_index(uint32_t* idx) = 0;
  virtual int transform(const float m[16], float bbox[6]) = 0;   // in place; the bounding box of the result
  virtual int normals() = 0;
  virtual int cluster(float nthr, float dthr, std::vector<Cluster>& table, uint64_t counters[3]) = 0;   // table in creation order
  virtual int behind(const float* reps4, size_t K, float dist, uint32_t* counts) = 0;
  virtual int cov(uint32_t cluster, const float rep[4], float inlier, double sums[10]) = 0;
};

Ops* make_host_ops();
int make_gpu_ops(int device, Ops** out);   // axis_align.hip; SF_ERR_DEVICE without a GPU
int& batch_size();                         // sf_axis_align_tune("batch")
int& profile();                            // sf_axis_align_tune("profile")

}  // namespace aa
}  // namespace sf
