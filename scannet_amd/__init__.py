"""scannet_amd -- MI355X-native RGB-D integration hot path of the ScanNet processing pipeline.

Host-side Python mirror of the reference interfaces for this path (SensReader, the TSDF `improve` stage,
Segmentator) over the C ABI of libscanfuse.so (include/scanfuse.h).  The compute path is hand-written HIP
for gfx950; importing a compute entry point without the built library raises (no CPU fallback).
"""
# Importing this package changes nothing in the process: the HIP runtime's GPU_MAX_HW_QUEUES (hardware queues per process, default 4) belongs to
# the environment the application runs in -- neither the package, the library nor its tools set it; sf_fuse_run leaves a note in sf_fuse_run_note()
# when it ran on fewer queues than streams.

__all__ = ["synth"]
