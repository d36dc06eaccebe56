"""Voxel-hash TSDF fuser -- host-side mirror of the scene-representation interface of the reference's
`improve` stage (external DepthSensing.exe, call site Server/scan_processor.py:137-138).

Thin ctypes layer over the C ABI (include/scanfuse.h); all arithmetic runs in the HIP kernels of
scannet_amd/csrc/fuser*.hip.  There is no CPU fallback: creating a Fuser without an MI355X raises.
"""
import ctypes as C

import numpy as np

from . import _abi
from ._abi import SfParams, SfStats, check

class SfRunStats(C.Structure):
    _fields_ = [("frames_total", C.c_uint64), ("frames_integrated", C.c_uint64), ("frames_skipped", C.c_uint64),
                ("decode_threads", C.c_uint32), ("color_fused", C.c_uint32),
                ("seconds_total", C.c_double), ("seconds_decode_cpu", C.c_double)]


VOXEL_DTYPE = np.dtype([("sdf", "<f4"), ("r", "u1"), ("g", "u1"), ("b", "u1"), ("w", "u1")])


def default_params(**over):
    """zParametersScanNet.txt values with BASELINE.json's 4 mm / 2^19-bucket overrides; keyword overrides."""
    p = SfParams()
    _abi.lib().sf_params_default(C.byref(p))
    for k, v in over.items():
        if not hasattr(p, k):
            raise AttributeError("sf_params has no field %r" % k)
        setattr(p, k, v)
    return p


def load_params(path, base=None):
    """Parse an mLib ParameterFile (e.g. Server/tools/recons/zParametersScanNet.txt)."""
    p = base if base is not None else default_params()
    check(_abi.lib().sf_params_load_file(str(path).encode(), C.byref(p)))
    return p


class SfRaycastParams(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32),
                ("fx", C.c_float), ("fy", C.c_float), ("mx", C.c_float), ("my", C.c_float),
                ("depth_min", C.c_float), ("depth_max", C.c_float),
                ("ray_increment_factor", C.c_float), ("thres_sample_dist_factor", C.c_float), ("thres_dist_factor", C.c_float),
                ("refine_iters", C.c_int32), ("reserved", C.c_int32 * 4)]


def default_raycast_params(**over):
    """sf_raycast_params_default (zParametersScanNet.txt's ray-cast values; size and intrinsics 0 = the fuser's); keyword overrides."""
    r = SfRaycastParams()
    L = _abi.lib()
    L.sf_raycast_params_default.argtypes = [C.POINTER(SfRaycastParams)]
    L.sf_raycast_params_default.restype = None
    L.sf_raycast_params_default(C.byref(r))
    for k, v in over.items():
        if not hasattr(r, k) or k == "reserved":
            raise AttributeError("sf_raycast_params has no field %r" % k)
        setattr(r, k, v)
    return r


def load_raycast_params(path, base=None):
    """The ray-cast keys (s_rayCastWidth / Height, s_renderDepthMin / Max, s_SDFRay*) of an mLib ParameterFile."""
    r = base if base is not None else default_raycast_params()
    L = _abi.lib()
    L.sf_raycast_params_load_file.argtypes = [C.c_char_p, C.POINTER(SfRaycastParams)]
    check(L.sf_raycast_params_load_file(str(path).encode(), C.byref(r)))
    return r


class SfTrackParams(C.Structure):
    _fields_ = [("levels", C.c_int32), ("max_iters", C.c_int32 * 4), ("dist_thres", C.c_float * 4), ("normal_thres", C.c_float * 4),
                ("early_out", C.c_float), ("min_correspondences", C.c_int32), ("max_translation", C.c_float), ("max_rotation", C.c_float),
                ("raycast", SfRaycastParams), ("colour_weight", C.c_float), ("colour_thres", C.c_float), ("colour_gradient_min", C.c_float),
                ("reserved", C.c_int32 * 5)]


class SfTrackResult(C.Structure):
    _fields_ = [("tracked", C.c_int32), ("iterations", C.c_int32 * 4), ("correspondences", C.c_int32), ("rms_residual", C.c_float),
                ("lost_reason", C.c_int32), ("colour_correspondences", C.c_int32), ("colour_rms_residual", C.c_float), ("reserved", C.c_int32 * 4)]

    def as_dict(self):
        return dict(tracked=bool(self.tracked), iterations=list(self.iterations), correspondences=int(self.correspondences),
                    rms_residual=float(self.rms_residual), lost_reason=int(self.lost_reason), colour_correspondences=int(self.colour_correspondences),
                    colour_rms_residual=float(self.colour_rms_residual))


def default_track_params(**over):
    """sf_track_params_default (DESIGN.md "Camera tracking"); keyword overrides (lists for the per-level fields)."""
    t = SfTrackParams()
    L = _abi.lib()
    L.sf_track_params_default.argtypes = [C.POINTER(SfTrackParams)]
    L.sf_track_params_default.restype = None
    L.sf_track_params_default(C.byref(t))
    for k, v in over.items():
        if not hasattr(t, k) or k == "reserved":
            raise AttributeError("sf_track_params has no field %r" % k)
        if k in ("max_iters", "dist_thres", "normal_thres"):
            arr = getattr(t, k)
            for i, x in enumerate(v):
                arr[i] = x
        else:
            setattr(t, k, v)
    return t


def load_track_params(path, base=None):
    """The tracking keys (s_maxLevels, s_maxOuterIter, s_distThres, s_normalThres, ...) of an mLib ParameterFile such as
    zParametersTrackingDefault.txt."""
    t = base if base is not None else default_track_params()
    L = _abi.lib()
    L.sf_track_params_load_file.argtypes = [C.c_char_p, C.POINTER(SfTrackParams)]
    check(L.sf_track_params_load_file(str(path).encode(), C.byref(t)))
    return t


class SfReintParams(C.Structure):
    _fields_ = [("max_frame_fixes", C.c_int32), ("top_n_active", C.c_int32), ("min_pose_dist_sqrt", C.c_float), ("reserved", C.c_int32 * 5)]


class SfReintStats(C.Structure):
    _fields_ = [("steps", C.c_uint64), ("frames_moved", C.c_uint64), ("frames_removed", C.c_uint64), ("frames_added", C.c_uint64),
                ("passes", C.c_uint64), ("seconds_total", C.c_double)]


def default_reint_params(**over):
    """sf_reint_params_default (the trajectory-manager keys of zParametersScanNet.txt:25-28: 30 / 30 / 0.0); keyword overrides."""
    r = SfReintParams()
    L = _abi.lib()
    L.sf_reint_params_default.argtypes = [C.POINTER(SfReintParams)]
    L.sf_reint_params_default.restype = None
    L.sf_reint_params_default(C.byref(r))
    for k, v in over.items():
        if not hasattr(r, k) or k == "reserved":
            raise AttributeError("sf_reint_params has no field %r" % k)
        setattr(r, k, v)
    return r


def load_reint_params(path, base=None):
    """s_maxFrameFixes, s_topNActive and s_minPoseDistSqrt of an mLib ParameterFile; absent keys leave the base as it is."""
    r = base if base is not None else default_reint_params()
    L = _abi.lib()
    L.sf_reint_params_load_file.argtypes = [C.c_char_p, C.POINTER(SfReintParams)]
    check(L.sf_reint_params_load_file(str(path).encode(), C.byref(r)))
    return r


class SfAlignParams(C.Structure):
    _fields_ = [("level", C.c_int32), ("down_width", C.c_int32), ("down_height", C.c_int32), ("max_iters", C.c_int32),
                ("dist_thres", C.c_float), ("normal_thres", C.c_float), ("depth_min", C.c_float), ("depth_max", C.c_float), ("early_out", C.c_float),
                ("min_pair_correspondences", C.c_int32), ("fixed_frame", C.c_int32),
                ("pair_max_dist", C.c_float), ("pair_max_angle", C.c_float), ("max_translation", C.c_float), ("max_rotation", C.c_float),
                ("colour_weight", C.c_float), ("colour_thres", C.c_float), ("colour_gradient_min", C.c_float),
                ("reserved", C.c_int32 * 6)]


class SfAlignResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("iterations", C.c_int32), ("pairs_used", C.c_int32), ("frames_unconnected", C.c_int32),
                ("frames_rejected", C.c_int32), ("reserved0", C.c_int32), ("correspondences", C.c_int64),
                ("rms_first", C.c_float), ("rms_last", C.c_float), ("colour_correspondences", C.c_int64),
                ("colour_rms_first", C.c_float), ("colour_rms_last", C.c_float), ("reserved", C.c_int32 * 2)]

    def as_dict(self):
        return dict(status=int(self.status), iterations=int(self.iterations), pairs_used=int(self.pairs_used),
                    frames_unconnected=int(self.frames_unconnected), frames_rejected=int(self.frames_rejected),
                    correspondences=int(self.correspondences), rms_first=float(self.rms_first), rms_last=float(self.rms_last),
                    colour_correspondences=int(self.colour_correspondences), colour_rms_first=float(self.colour_rms_first),
                    colour_rms_last=float(self.colour_rms_last))


def default_align_params(**over):
    """sf_align_params_default (DESIGN.md "Global alignment"); keyword overrides."""
    a = SfAlignParams()
    L = _abi.lib()
    L.sf_align_params_default.argtypes = [C.POINTER(SfAlignParams)]
    L.sf_align_params_default.restype = None
    L.sf_align_params_default(C.byref(a))
    for k, v in over.items():
        if not hasattr(a, k) or k == "reserved":
            raise AttributeError("sf_align_params has no field %r" % k)
        setattr(a, k, v)
    return a


def load_align_params(path, base=None):
    """The dense-term keys (s_denseDistThresh, s_denseNormalThresh, s_denseColorThresh, s_denseColorGradientMin, s_denseDepthMin / Max, s_downsampledWidth / Height,
    s_numGlobalNonLinIterations) of an mLib ParameterFile such as zParametersBundlingScanNet.txt; absent keys leave the base as it is."""
    a = base if base is not None else default_align_params()
    L = _abi.lib()
    L.sf_align_params_load_file.argtypes = [C.c_char_p, C.POINTER(SfAlignParams)]
    check(L.sf_align_params_load_file(str(path).encode(), C.byref(a)))
    return a


def align_pairs(poses, params=None, capacity=4096):
    """sf_align_pairs (host only): the default pair list of K keyframe poses ([K,16] / [K,4,4] camToWorld) -> (int32 [min(count, capacity), 2] of
    (source, target), the count the rule produces)."""
    a = params if params is not None else default_align_params()
    poses = np.ascontiguousarray(poses, dtype=np.float32).reshape(-1, 16)
    out = np.zeros((max(int(capacity), 1), 2), np.int32)
    n = C.c_uint64(0)
    L = _abi.lib()
    L.sf_align_pairs.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(SfAlignParams), C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    check(L.sf_align_pairs(_ptr(poses), len(poses), C.byref(a), _ptr(out), int(capacity), C.byref(n)))
    return out[:min(n.value, int(capacity))].copy(), int(n.value)


def align_spread(poses, keyframes, new_key_poses):
    """sf_align_spread (host only): the keyframes' correction carried to every frame of the trajectory -> float32 [n,16]."""
    poses = np.ascontiguousarray(poses, dtype=np.float32).reshape(-1, 16)
    keys = np.ascontiguousarray(keyframes, dtype=np.uint64)
    new = np.ascontiguousarray(new_key_poses, dtype=np.float32).reshape(-1, 16)
    if len(keys) != len(new):
        raise ValueError("one new pose per keyframe")
    out = np.empty_like(poses)
    L = _abi.lib()
    L.sf_align_spread.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    check(L.sf_align_spread(_ptr(poses), len(poses), _ptr(keys), len(keys), _ptr(new), _ptr(out)))
    return out


class SfAlignScanParams(C.Structure):
    _fields_ = [("group_size", C.c_int32), ("top_frames", C.c_int32), ("reserved", C.c_int32 * 6)]


class SfAlignScanResult(C.Structure):
    _fields_ = [("levels", C.c_int32), ("groups", C.c_int32), ("groups_status", C.c_int32 * 3), ("max_iterations", C.c_int32),
                ("frames_unconnected", C.c_int32), ("frames_rejected", C.c_int32), ("correspondences", C.c_int64), ("top", SfAlignResult),
                ("reserved", C.c_int32 * 4)]

    def as_dict(self):
        return dict(levels=int(self.levels), groups=int(self.groups), groups_status=[int(x) for x in self.groups_status],
                    max_iterations=int(self.max_iterations), frames_unconnected=int(self.frames_unconnected),
                    frames_rejected=int(self.frames_rejected), correspondences=int(self.correspondences), top=self.top.as_dict())


def default_align_scan_params(**over):
    """sf_align_scan_params_default: group_size 16, top_frames 256; keyword overrides."""
    s = SfAlignScanParams()
    L = _abi.lib()
    L.sf_align_scan_params_default.argtypes = [C.POINTER(SfAlignScanParams)]
    L.sf_align_scan_params_default.restype = None
    L.sf_align_scan_params_default(C.byref(s))
    for k, v in over.items():
        if k not in ("group_size", "top_frames"):
            raise AttributeError("sf_align_scan_params has no field %r" % k)
        setattr(s, k, int(v))
    return s


def align_scan_plan(poses, params=None, scan=None, members_capacity=None, groups_capacity=None, top_capacity=None):
    """sf_align_scan_plan (host only): the groups and the top of K keyframe poses -> dict(members int32 [M], group_first int32 [G + 1], group_level
    int32 [G], top int32 [T], levels, counts (M, G, T) as the rule gives them; the arrays stop at the capacities, which default to what the rule can give)."""
    a = params if params is not None else default_align_params()
    sp = scan if scan is not None else default_align_scan_params()
    poses = np.ascontiguousarray(poses, dtype=np.float32).reshape(-1, 16)
    K = len(poses)
    mc = 2 * K + 16 if members_capacity is None else int(members_capacity)
    gc = K + 1 if groups_capacity is None else int(groups_capacity)
    tc = K if top_capacity is None else int(top_capacity)
    members, first, level, top = np.zeros(max(mc, 1), np.int32), np.zeros(gc + 1, np.int32), np.zeros(max(gc, 1), np.int32), np.zeros(max(tc, 1), np.int32)
    nm, ng, nt, levels = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_int32(0)
    L = _abi.lib()
    L.sf_align_scan_plan.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(SfAlignParams), C.POINTER(SfAlignScanParams), C.c_void_p, C.c_uint64, C.c_void_p,
                                     C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                     C.POINTER(C.c_int32)]
    check(L.sf_align_scan_plan(_ptr(poses), K, C.byref(a), C.byref(sp), _ptr(members), mc, _ptr(first), _ptr(level), gc, _ptr(top), tc, C.byref(nm), C.byref(ng),
                               C.byref(nt), C.byref(levels)))
    g = min(ng.value, gc)
    return dict(members=members[:min(nm.value, mc)].copy(), group_first=first[:g + 1].copy(), group_level=level[:g].copy(), top=top[:min(nt.value, tc)].copy(),
                levels=int(levels.value), counts=(int(nm.value), int(ng.value), int(nt.value)))


def align_keyframes(poses, every):
    """Every `every`-th of the frames with a finite pose (rows 0..2), in frame order, starting with the first -> uint64 frame indices."""
    poses = np.asarray(poses, dtype=np.float32).reshape(-1, 16)
    good = np.flatnonzero(np.isfinite(poses[:, :12]).all(axis=1))
    return good[::max(1, int(every))].astype(np.uint64)


ALIGN_COLOUR_WEIGHT = 0.1   # the working weight of the colour term (DESIGN.md 4f has the sweep); sf_align_params_default keeps 0, the term off


def align_and_reintegrate(fuser, sensor_data, integrated, every=10, params=None, reint_params=None, colour=False, with_colour=False, colour_weight=None,
                          group=None, top=None):
    """The correction loop: keyframes are every `every`-th frame with a finite integrated pose; their depth is decoded, the default pairs built, the
    keyframes aligned (Fuser.align), the correction spread over the trajectory, and the volume moved there (Fuser.update_trajectory, which updates a
    float32 C-contiguous `integrated` in place).  with_colour: the keyframes' colour pictures are decoded too and the aligner runs its colour term
     with `colour_weight` (None: the parameters' own when positive, else ALIGN_COLOUR_WEIGHT).  `colour` is the re-integration's:
    the file's colour frames go back into the volume with the depth.  -> (target poses float32 [n,16], SfAlignResult, re-integration statistics).
    group / top: sf_align_scan_params' group_size / top_frames.  With more keyframes than the top takes (256 unless `top` says otherwise), or when
    either is given, the keyframes go through Fuser.align_scan and the second value is its SfAlignScanResult."""
    a = params if params is not None else default_align_params()
    if with_colour:
        b = SfAlignParams.from_buffer_copy(a)
        b.colour_weight = float(colour_weight) if colour_weight is not None else (a.colour_weight if a.colour_weight > 0 else ALIGN_COLOUR_WEIGHT)
        a = b
    cur = np.ascontiguousarray(integrated, dtype=np.float32).reshape(-1, 16)
    keys = align_keyframes(cur, every)
    if len(keys) < 2:
        raise ValueError("alignment needs two keyframes, the trajectory has %d" % len(keys))
    depth = np.stack([np.ascontiguousarray(sensor_data.frames[int(k)].decompress_depth(), dtype=np.uint16).reshape(-1) for k in keys])
    rgb = None
    if with_colour:
        rgb = np.stack([np.ascontiguousarray(sensor_data.frames[int(k)].decompress_color(), dtype=np.uint8).reshape(-1) for k in keys])
    scan = default_align_scan_params(**{k: v for k, v in (("group_size", group), ("top_frames", top)) if v is not None})
    pairs, count = align_pairs(cur[keys.astype(np.int64)], a)
    if group is not None or top is not None or len(keys) > scan.top_frames or count > len(pairs):
        new, res = fuser.align_scan(depth, cur[keys.astype(np.int64)], a, scan, rgb=rgb)
    else:
        new, res = fuser.align(depth, cur[keys.astype(np.int64)], pairs, a, rgb=rgb)
    target = align_spread(cur, keys, new)
    _, stats = fuser.update_trajectory(sensor_data, integrated, target, params=reint_params, colour=colour)
    return target, res, stats


def plan_reintegration(integrated, target, params=None, capacity=None):
    """sf_reint_plan: one step of the trajectory manager (host only).  integrated / target: [n,16] or [n,4,4] camToWorld, what the volume holds and
    what it should hold (all -inf: not in the volume / lost) -> the frames to re-integrate now (uint64 array, largest pose change first)."""
    r = params if params is not None else default_reint_params()
    a = np.ascontiguousarray(integrated, dtype=np.float32).reshape(-1, 16)
    b = np.ascontiguousarray(target, dtype=np.float32).reshape(-1, 16)
    if a.shape != b.shape:
        raise ValueError("integrated and target trajectories differ in length")
    cap = int(capacity) if capacity is not None else max(0, min(int(r.max_frame_fixes), int(r.top_n_active)))
    out = np.zeros(max(cap, 1), np.uint64)
    n = C.c_uint64(0)
    L = _abi.lib()
    L.sf_reint_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(SfReintParams), C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    check(L.sf_reint_plan(_ptr(a), _ptr(b), len(a), C.byref(r), _ptr(out), cap, C.byref(n)))
    return out[:n.value].copy()


TRACK_COLOUR_WEIGHT = 0.1   # the working weight of the tracker's colour term (DESIGN.md 4g has the sweep); sf_track_params_default keeps 0, the term off


def track_and_fuse(fuser, frames, first_pose, params=None, with_colour=False, colour_weight=None):
    """Frame-to-model tracking loop: frame 0 is fused at first_pose, every later frame is tracked against the volume so far, starting from the last
    tracked pose, and fused at the pose found; a lost frame is not fused.  frames: iterable of u16 depth [H,W] (or (depth, rgb) pairs).
    with_colour: the frames are (depth, rgb) pairs and every track takes the frame's picture: sf_fuser_track_rgbd, the colour term of DESIGN.md 4g with
    `colour_weight` (None: the parameters' own when positive, else TRACK_COLOUR_WEIGHT).
    -> list of poses (float32 [4,4]; all -inf where lost) and the list of result dicts (None for frame 0)."""
    if with_colour:
        t = params if params is not None else default_track_params()
        params = SfTrackParams.from_buffer_copy(t)
        params.colour_weight = float(colour_weight) if colour_weight is not None else (t.colour_weight if t.colour_weight > 0 else TRACK_COLOUR_WEIGHT)
    poses, results = [], []
    last = np.ascontiguousarray(first_pose, dtype=np.float32).reshape(4, 4)
    for k, fr in enumerate(frames):
        depth, rgb = fr if isinstance(fr, tuple) else (fr, None)
        if k == 0:
            pose, res = last, None
        else:
            if with_colour and rgb is None:
                raise ValueError("track_and_fuse(with_colour=True): frame %d has no picture" % k)
            pose, res = fuser.track(depth, last, params=params, rgb=rgb if with_colour else None)
            res = res.as_dict()
        if pose is None:
            poses.append(np.full((4, 4), -np.inf, np.float32))
        else:
            fuser.integrate(depth, pose, rgb=rgb)
            poses.append(pose)
            last = pose
        results.append(res)
    return poses, results


def device_count():
    n = C.c_int(0)
    rc = _abi.lib().sf_device_count(C.byref(n))
    return n.value if rc == 0 else 0


def _ptr(a):
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data_as(C.c_void_p)
    if hasattr(a, "data_ptr"):  # torch tensor
        return C.c_void_p(a.data_ptr())
    return C.c_void_p(int(a))


class Fuser:
    def __init__(self, params=None, device=0, **tune):
        self.params = params if params is not None else default_params()
        self.device = device
        h = C.c_void_p()
        check(_abi.lib().sf_fuser_create(C.byref(self.params), int(device), C.byref(h)))
        self._h = h
        self.tune(**tune)

    def tune(self, **switches):
        """Scheduling switches (include/scanfuse_internal.h sf_fuser_tune: batch, overlap, xcd_walk, pipe, pipe_overlap, front_prio,
        front_lo_lowest, alloc_group, alloc_ray, brick_cache, tail_wide); the voxels are bit-identical under all of them -- bench.py and
        the tests use this, a pipeline stage never needs to."""
        L = _abi.lib()
        L.sf_fuser_tune.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
        for k, v in switches.items():
            check(L.sf_fuser_tune(self._h, k.encode(), int(v)))
        return self

    def close(self):
        if getattr(self, "_h", None):
            _abi.lib().sf_fuser_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- host buffers -------------------------------------------------------------------------------
    def _host_frame(self, fn, depth, pose, rgb):
        depth = np.ascontiguousarray(depth, dtype=np.uint16)
        if depth.size != self.params.depth_width * self.params.depth_height:
            raise ValueError("depth frame has %d pixels, fuser expects %dx%d" % (depth.size, self.params.depth_width, self.params.depth_height))
        pose = np.ascontiguousarray(pose, dtype=np.float32).reshape(16)
        if rgb is not None:
            rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
            want = (self.params.color_width * self.params.color_height if self.params.color_width > 0 else depth.size) * 3
            if rgb.size != want:
                raise ValueError("rgb must be HxWx3 at depth resolution (or at the colour resolution given in sf_params)")
        rc = check(fn(self._h, _ptr(depth), _ptr(rgb), _ptr(pose)), allow=(_abi.SF_ERR_SKIPPED,))
        return rc == 0

    def integrate(self, depth, pose, rgb=None):
        """Fuse one frame; returns False when the frame was skipped (pose all -inf)."""
        return self._host_frame(_abi.lib().sf_fuser_integrate, depth, pose, rgb)

    def deintegrate(self, depth, pose, rgb=None):
        return self._host_frame(_abi.lib().sf_fuser_deintegrate, depth, pose, rgb)

    # -- device buffers (torch tensors or raw device pointers) --------------------------------------
    def integrate_device(self, d_depth, pose, d_rgb=None):
        pose = np.ascontiguousarray(pose, dtype=np.float32).reshape(16)
        rc = check(_abi.lib().sf_fuser_integrate_device(self._h, _ptr(d_depth), _ptr(d_rgb), _ptr(pose)), allow=(_abi.SF_ERR_SKIPPED,))
        return rc == 0

    def deintegrate_device(self, d_depth, pose, d_rgb=None):
        pose = np.ascontiguousarray(pose, dtype=np.float32).reshape(16)
        rc = check(_abi.lib().sf_fuser_deintegrate_device(self._h, _ptr(d_depth), _ptr(d_rgb), _ptr(pose)), allow=(_abi.SF_ERR_SKIPPED,))
        return rc == 0

    def integrate_batch_device(self, d_depth, frame_stride_bytes, poses, d_rgb=None, rgb_stride_bytes=0):
        poses = np.ascontiguousarray(poses, dtype=np.float32).reshape(-1, 16)
        if d_rgb is None:
            check(_abi.lib().sf_fuser_integrate_batch_device(self._h, _ptr(d_depth), int(frame_stride_bytes), _ptr(poses), len(poses)))
        else:
            L = _abi.lib()
            L.sf_fuser_integrate_batch_device_rgb.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]
            check(L.sf_fuser_integrate_batch_device_rgb(self._h, _ptr(d_depth), int(frame_stride_bytes), _ptr(d_rgb), int(rgb_stride_bytes), _ptr(poses), len(poses)))

    # -- re-integration of frames whose poses were revised ---------------------------------
    def reintegrate(self, depth, old_pose, new_pose, rgb=None):
        """Take one frame (host buffers) out of the volume at old_pose and put it back at new_pose in one pass (sf_fuser_reintegrate); an all -inf
        old / new pose: only put in / only taken out.  False when both are all -inf (nothing done)."""
        depth = np.ascontiguousarray(depth, dtype=np.uint16)
        if depth.size != self.params.depth_width * self.params.depth_height:
            raise ValueError("depth frame has %d pixels, fuser expects %dx%d" % (depth.size, self.params.depth_width, self.params.depth_height))
        old_pose = np.ascontiguousarray(old_pose, dtype=np.float32).reshape(16)
        new_pose = np.ascontiguousarray(new_pose, dtype=np.float32).reshape(16)
        if rgb is not None:
            rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
            want = (self.params.color_width * self.params.color_height if self.params.color_width > 0 else depth.size) * 3
            if rgb.size != want:
                raise ValueError("rgb must be HxWx3 at depth resolution (or at the colour resolution given in sf_params)")
        L = _abi.lib()
        L.sf_fuser_reintegrate.argtypes = [C.c_void_p] * 5
        return check(L.sf_fuser_reintegrate(self._h, _ptr(depth), _ptr(rgb), _ptr(old_pose), _ptr(new_pose)), allow=(_abi.SF_ERR_SKIPPED,)) == 0

    def reintegrate_batch_device(self, d_depth, frame_stride_bytes, old_poses, new_poses, d_rgb=None, rgb_stride_bytes=0):
        """n device-resident frames: for each in order, deintegrate at old_poses[j], integrate at new_poses[j] -- bit for bit that sequence, as
        mixed-sign passes of up to batch_frames operations (sf_fuser_reintegrate_batch_device)."""
        old_poses = np.ascontiguousarray(old_poses, dtype=np.float32).reshape(-1, 16)
        new_poses = np.ascontiguousarray(new_poses, dtype=np.float32).reshape(-1, 16)
        if old_poses.shape != new_poses.shape:
            raise ValueError("old and new poses differ in number")
        L = _abi.lib()
        L.sf_fuser_reintegrate_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64]
        check(L.sf_fuser_reintegrate_batch_device(self._h, _ptr(d_depth), int(frame_stride_bytes), _ptr(d_rgb), int(rgb_stride_bytes), _ptr(old_poses),
                                                  _ptr(new_poses), len(old_poses)))

    def update_trajectory(self, sensor_data, integrated, target, params=None, max_steps=0, colour=False, decode_threads=0):
        """sf_fuse_update_trajectory: steps of the trajectory manager over a scannet_amd.sens.SensorData until nothing is left to move (max_steps 0)
        or max_steps are done.  integrated ([n,16] / [n,4,4] float32, what the volume holds) is updated IN PLACE when it is a C-contiguous float32
        array; the updated trajectory [n,16] and the run's statistics are returned either way."""
        r = params if params is not None else default_reint_params()
        cur = integrated if (isinstance(integrated, np.ndarray) and integrated.dtype == np.float32 and integrated.flags.c_contiguous) \
            else np.array(integrated, dtype=np.float32)
        tgt = np.ascontiguousarray(target, dtype=np.float32).reshape(-1, 16)
        if cur.size != tgt.size:
            raise ValueError("integrated and target trajectories differ in length")
        st = SfReintStats()
        L = _abi.lib()
        L.sf_fuse_update_trajectory.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(SfReintParams), C.c_uint64, C.c_int, C.c_int,
                                                C.POINTER(SfReintStats)]
        check(L.sf_fuse_update_trajectory(self._h, sensor_data._h, _ptr(cur), _ptr(tgt), C.byref(r), int(max_steps), int(bool(colour)), int(decode_threads),
                                          C.byref(st)))
        return cur.reshape(-1, 16), {k: getattr(st, k) for k, _ in SfReintStats._fields_}

    @property
    def batch_frames(self):
        """Frames fused per pass over the voxel tiles by integrate_batch_device / run (default 16; tune(batch=...))."""
        return int(_abi.lib().sf_fuser_batch_frames(self._h))

    def reset(self):
        """Empty volume again; parameters, streams and tuning stay (sf_fuser_reset)."""
        L = _abi.lib()
        L.sf_fuser_reset.argtypes = [C.c_void_p]
        check(L.sf_fuser_reset(self._h))

    def garbage_collect(self):
        n = C.c_uint32(0)
        check(_abi.lib().sf_fuser_garbage_collect(self._h, C.byref(n)))
        return n.value

    def sync(self):
        check(_abi.lib().sf_fuser_sync(self._h))

    @property
    def stream(self):
        return _abi.lib().sf_fuser_stream(self._h)

    def stats(self):
        s = SfStats()
        check(_abi.lib().sf_fuser_stats(self._h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in SfStats._fields_}

    def profile(self, on=True):
        check(_abi.lib().sf_fuser_profile_enable(self._h, 1 if on else 0))

    def profile_read(self):
        ms, n, b = C.c_double(0), C.c_uint64(0), C.c_uint64(0)
        check(_abi.lib().sf_fuser_profile_read(self._h, C.byref(ms), C.byref(n), C.byref(b)))
        return ms.value, n.value, b.value

    def calib_tile_rmw(self, read_only=False, iters=20):
        """(average microseconds, tiles): the most recent pass's tile traffic without its arithmetic (pattern ceiling)."""
        us, n = C.c_double(0), C.c_uint32(0)
        check(_abi.lib().sf_fuser_calib_tile_rmw(self._h, 1 if read_only else 0, int(iters), C.byref(us), C.byref(n)))
        return us.value, n.value

    def calib_tile_rmw_ex(self, read_only=False, contiguous=False, tiles_per_turnaround=1, iters=10):
        """(average microseconds, tiles) of the most recent pass's tile traffic taken apart: scattered list or one contiguous span, G tiles read before G written."""
        L = _abi.lib()
        L.sf_fuser_calib_tile_rmw_ex.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint32)]
        mode = (1 if read_only else 0) | (2 if contiguous else 0) | ({1: 0, 2: 1, 4: 2}[int(tiles_per_turnaround)] << 2)
        us, n = C.c_double(0), C.c_uint32(0)
        check(L.sf_fuser_calib_tile_rmw_ex(self._h, mode, int(iters), C.byref(us), C.byref(n)))
        return us.value, n.value

    @staticmethod
    def prepare_run(sensor_data, params, device=0):
        """sf_fuse_run_prepare: with the file open and BEFORE the Fuser is created, start making the streams and rings a run of this file wants."""
        L = _abi.lib()
        L.sf_fuse_run_prepare.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        check(L.sf_fuse_run_prepare(sensor_data._h, C.byref(params), int(device)))

    def run(self, sensor_data, first=0, last=0, decode_threads=0):
        """Fuse frames [first, last) of a scannet_amd.sens.SensorData (threaded decode overlapped with the GPU)."""
        st = SfRunStats()
        check(_abi.lib().sf_fuse_run(self._h, sensor_data._h, int(first), int(last), int(decode_threads), C.byref(st)))
        out = {k: getattr(st, k) for k, _ in SfRunStats._fields_}
        L = _abi.lib()
        if hasattr(L, "sf_fuse_run_device_counts"):   # scanfuse_internal.h: where the frames were decoded
            c = (C.c_uint64 * 4)()
            L.sf_fuse_run_device_counts.argtypes = [C.POINTER(C.c_uint64)]
            check(L.sf_fuse_run_device_counts(c))
            out.update(depth_inflated_on_device=c[0], depth_inflated_on_host=c[1], jpeg_entropy_on_device=c[2], jpeg_entropy_on_host=c[3])
        return out

    # -- one large scan over several GPUs (scannet_amd/partition.py) -------------------------------------
    def set_slab(self, axis, lo_block, hi_block):
        """Only allocate blocks with lo_block <= coord[axis] < hi_block (axis < 0: no partition)."""
        check(_abi.lib().sf_fuser_set_slab(self._h, int(axis), int(lo_block), int(hi_block)))

    def export_blocks_where(self, axis, lo, hi, include_ghosts=False):
        """Live blocks with lo <= coord[axis] < hi -> (coords int32 [n,3], voxels VOXEL_DTYPE [n,512]), sorted by (x,y,z)."""
        L = _abi.lib()
        n = C.c_uint64(0)
        check(L.sf_fuser_export_blocks_where(self._h, int(axis), int(lo), int(hi), int(bool(include_ghosts)), None, None, 0, C.byref(n), 0))
        coords = np.zeros((n.value, 3), np.int32)
        vox = np.zeros((n.value, 512), VOXEL_DTYPE)
        if n.value:
            check(L.sf_fuser_export_blocks_where(self._h, int(axis), int(lo), int(hi), int(bool(include_ghosts)), _ptr(coords), _ptr(vox), n.value, C.byref(n), 0))
        order = np.lexsort((coords[:, 2], coords[:, 1], coords[:, 0]))
        return coords[order], vox[order]

    def import_blocks(self, coords, voxels, ghost=True):
        coords = np.ascontiguousarray(coords, np.int32).reshape(-1, 3)
        voxels = np.ascontiguousarray(voxels)
        if voxels.nbytes != len(coords) * 4096:
            raise ValueError("voxels must hold 4096 bytes per block")
        check(_abi.lib().sf_fuser_import_blocks(self._h, _ptr(coords), _ptr(voxels), len(coords), int(bool(ghost)), 0))

    def set_stripes(self, axis, origin_block, thickness_blocks, world, rank):
        """Own the stripes floor((coord[axis] - origin) / thickness) mod world == rank (sf_fuser_set_stripes)."""
        check(_abi.lib().sf_fuser_set_stripes(self._h, int(axis), int(origin_block), int(thickness_blocks), int(world), int(rank)))

    def count_boundary(self):
        n = C.c_uint64(0)
        check(_abi.lib().sf_fuser_export_boundary(self._h, None, None, 0, C.byref(n), 0))
        return n.value

    def export_boundary(self, coords=None, voxels=None):
        """The lowest block layer of each of this fuser's slabs / stripes.  Without arguments: numpy (coords int32 [n,3], voxels
        VOXEL_DTYPE [n,512]).  With `coords` / `voxels` = device buffers (torch CUDA tensors or raw pointers, at least count_boundary()
        blocks): written in place on the GPU, returns n -- nothing touches host memory."""
        L = _abi.lib()
        n = C.c_uint64(0)
        if coords is None:
            m = self.count_boundary()
            c = np.zeros((m, 3), np.int32)
            v = np.zeros((m, 512), VOXEL_DTYPE)
            if m:
                check(L.sf_fuser_export_boundary(self._h, _ptr(c), _ptr(v), m, C.byref(n), 0))
            return c, v
        cap = coords.shape[0] if hasattr(coords, "shape") else self.count_boundary()
        check(L.sf_fuser_export_boundary(self._h, _ptr(coords), _ptr(voxels), int(cap), C.byref(n), 1))
        return n.value

    def import_ghosts(self, coords, voxels, n=None):
        """Of a (gathered) payload keep the blocks this fuser needs as ghosts.  numpy arrays or device buffers; returns how many were kept."""
        L = _abi.lib()
        on_dev = not isinstance(coords, np.ndarray)
        if not on_dev:
            coords = np.ascontiguousarray(coords, np.int32).reshape(-1, 3)
            voxels = np.ascontiguousarray(voxels)
        cnt = int(coords.shape[0] if n is None else n)
        got = C.c_uint64(0)
        check(L.sf_fuser_import_ghosts(self._h, _ptr(coords), _ptr(voxels), cnt, 1 if on_dev else 0, C.byref(got)))
        return got.value

    def mc_timing(self):
        """Phases of the most recent extract_mesh() in ms (scanfuse_internal.h sf_fuser_mc_timing) + block / triangle / vertex counts."""
        L = _abi.lib()
        L.sf_fuser_mc_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int]
        t = (C.c_double * 12)()
        check(L.sf_fuser_mc_timing(self._h, t, 12))
        names = ("total", "live_list", "count_pass", "scan_emit_pass", "vertex_sort", "heads_scan_weld", "triangle_sort_gather", "downloads_device", "host_alloc_and_wait")
        out = {k: round(t[i], 3) for i, k in enumerate(names)}
        out.update(blocks=int(t[9]), triangles=int(t[10]), vertices=int(t[11]))
        return out

    def extract_mesh(self):
        """Marching cubes over all live blocks -> segmentator.Mesh (vertices in edge-key order, deterministic)."""
        from .segmentator import Mesh
        h = C.c_void_p()
        check(_abi.lib().sf_fuser_extract_mesh(self._h, C.byref(h)))
        return Mesh(h)

    # -- ray casting (DESIGN.md "Ray casting") ---------------------------------------------------------
    def raycast_size(self, params=None):
        """(width, height) of the images raycast() / raycast_device() make with these parameters (sf_fuser_raycast_size; invalid ones raise)."""
        r = params if params is not None else default_raycast_params()
        L = _abi.lib()
        L.sf_fuser_raycast_size.argtypes = [C.c_void_p, C.POINTER(SfRaycastParams), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        w, h = C.c_int32(0), C.c_int32(0)
        check(L.sf_fuser_raycast_size(self._h, C.byref(r), C.byref(w), C.byref(h)))
        return w.value, h.value

    def raycast(self, pose, params=None, normals=True, color=True):
        """Ray-cast the volume from camToWorld `pose` -> (depth [H,W] f32 metres along camera z, normals [H,W,3] f32 world frame or None,
        rgb [H,W,3] u8 or None).  Misses: depth and normal -inf, colour 0."""
        r = params if params is not None else default_raycast_params()
        W, H = self.raycast_size(r)
        pose = np.ascontiguousarray(pose, dtype=np.float32).reshape(16)
        depth = np.empty((H, W), np.float32)
        nrm = np.empty((H, W, 3), np.float32) if normals else None
        rgb = np.empty((H, W, 3), np.uint8) if color else None
        L = _abi.lib()
        L.sf_fuser_raycast.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(SfRaycastParams), C.c_void_p, C.c_void_p, C.c_void_p]
        check(L.sf_fuser_raycast(self._h, _ptr(pose), C.byref(r), _ptr(depth), _ptr(nrm), _ptr(rgb)))
        return depth, nrm, rgb

    def raycast_device(self, poses, d_depth=None, d_normals=None, d_rgb=None, params=None):
        """n poses ([n,16] or [n,4,4], host) -> device buffers (torch tensors or raw pointers), image after image: depth n*H*W f32,
        normals n*H*W*3 f32, rgb n*H*W*3 u8; any may be None.  Queued on self.stream, returns without waiting."""
        r = params if params is not None else default_raycast_params()
        poses = np.ascontiguousarray(poses, dtype=np.float32).reshape(-1, 16)
        L = _abi.lib()
        L.sf_fuser_raycast_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(SfRaycastParams), C.c_void_p, C.c_void_p, C.c_void_p]
        check(L.sf_fuser_raycast_device(self._h, _ptr(poses), len(poses), C.byref(r), _ptr(d_depth), _ptr(d_normals), _ptr(d_rgb)))

    # -- global alignment (DESIGN.md "Global alignment") ----------------------------------------------
    def _align_args(self, poses, pairs, params):
        a = params if params is not None else default_align_params()
        poses = np.ascontiguousarray(poses, dtype=np.float32).reshape(-1, 16)
        pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        return a, poses, pairs

    def _align_rgb(self, rgb, K):
        """K RGB8 pictures at the size the fuser fuses colour at (color_width x color_height, else the size of the depth frames given to it), contiguous."""
        rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
        p = self.params
        cw, ch = (p.color_width, p.color_height) if p.color_width > 0 and p.color_height > 0 else (p.depth_width, p.depth_height)
        if rgb.size != K * cw * ch * 3:
            raise ValueError("rgb holds %d bytes, %d pictures of %dx%dx3 expected" % (rgb.size, K, cw, ch))
        return rgb

    def align(self, depth, poses, pairs, params=None, rgb=None):
        """sf_fuser_align: K u16 keyframes (host, [K, H*W] at the fuser's input size) with camToWorld poses [K,16] aligned jointly over the directed
        pairs [P,2] (source, target).  rgb: the keyframes' RGB8 pictures ([K, h*w*3] at the size the fuser fuses colour at, color_width x color_height, else
        the depth frames' own size): sf_fuser_align_rgbd, the
        colour term of DESIGN.md 4f with the parameters' colour_weight.  -> (poses float32 [K,16], SfAlignResult)."""
        a, poses, pairs = self._align_args(poses, pairs, params)
        depth = np.ascontiguousarray(depth, dtype=np.uint16)
        if depth.size != len(poses) * self.params.depth_width * self.params.depth_height:
            raise ValueError("depth holds %d pixels, %d frames of %dx%d expected" % (depth.size, len(poses), self.params.depth_width, self.params.depth_height))
        out = np.empty_like(poses)
        res = SfAlignResult()
        L = _abi.lib()
        if rgb is not None:
            rgb = self._align_rgb(rgb, len(poses))
            L.sf_fuser_align_rgbd.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(SfAlignParams),
                                              C.c_void_p, C.POINTER(SfAlignResult)]
            check(L.sf_fuser_align_rgbd(self._h, _ptr(depth), _ptr(rgb), len(poses), _ptr(poses), _ptr(pairs), len(pairs), C.byref(a), _ptr(out), C.byref(res)))
            return out, res
        L.sf_fuser_align.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(SfAlignParams), C.c_void_p,
                                     C.POINTER(SfAlignResult)]
        check(L.sf_fuser_align(self._h, _ptr(depth), len(poses), _ptr(poses), _ptr(pairs), len(pairs), C.byref(a), _ptr(out), C.byref(res)))
        return out, res

    def align_device(self, d_depth, frame_stride_bytes, poses, pairs, params=None, d_rgb=None, rgb_stride_bytes=0):
        """align() for keyframes already in HBM (torch tensor or raw pointer), `frame_stride_bytes` apart, read on self.stream.  d_rgb: the
        keyframes' pictures in HBM, `rgb_stride_bytes` apart (sf_fuser_align_rgbd_device)."""
        a, poses, pairs = self._align_args(poses, pairs, params)
        out = np.empty_like(poses)
        res = SfAlignResult()
        L = _abi.lib()
        if d_rgb is not None:
            L.sf_fuser_align_rgbd_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64,
                                                     C.POINTER(SfAlignParams), C.c_void_p, C.POINTER(SfAlignResult)]
            check(L.sf_fuser_align_rgbd_device(self._h, _ptr(d_depth), int(frame_stride_bytes), _ptr(d_rgb),
                                               int(rgb_stride_bytes), len(poses), _ptr(poses), _ptr(pairs), len(pairs), C.byref(a), _ptr(out), C.byref(res)))
            return out, res
        L.sf_fuser_align_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(SfAlignParams),
                                            C.c_void_p, C.POINTER(SfAlignResult)]
        check(L.sf_fuser_align_device(self._h, _ptr(d_depth), int(frame_stride_bytes), len(poses), _ptr(poses), _ptr(pairs), len(pairs), C.byref(a),
                                      _ptr(out), C.byref(res)))
        return out, res

    def _staged(self, host):
        """A host array's copy in HBM (sf_device_malloc / sf_device_upload) -> the device pointer; the caller frees it with sf_device_free."""
        L = _abi.lib()
        d = C.c_void_p()
        check(L.sf_device_malloc(int(self.device), host.nbytes, C.byref(d)))
        rc = L.sf_device_upload(d, _ptr(host), host.nbytes)
        if rc != 0:
            L.sf_device_free(d)
            check(rc)
        return d

    def align_groups(self, depth, members, group_first, poses, params=None, rgb=None):
        """sf_fuser_align_groups_device on host arrays (staged through sf_device_upload): K u16 keyframes [K, H*W], the groups' frames `members` [M] with
        group_first [G + 1], one pose per member slot [M,16]; rgb: the K pictures (the colour term) -> (poses float32 [M,16], [SfAlignResult] * G)."""
        a = params if params is not None else default_align_params()
        depth = np.ascontiguousarray(depth, dtype=np.uint16)
        px = self.params.depth_width * self.params.depth_height
        if depth.size % px or depth.size == 0:
            raise ValueError("depth holds %d pixels, frames of %dx%d expected" % (depth.size, self.params.depth_width, self.params.depth_height))
        K = depth.size // px
        members = np.ascontiguousarray(members, dtype=np.int32).reshape(-1)
        group_first = np.ascontiguousarray(group_first, dtype=np.int32).reshape(-1)
        poses = np.ascontiguousarray(poses, dtype=np.float32).reshape(-1, 16)
        G = len(group_first) - 1
        if G < 1 or group_first[G] != len(members) or len(poses) != len(members):
            raise ValueError("group_first must end at the %d member slots, which have one pose each (%d given)" % (len(members), len(poses)))
        out = np.empty_like(poses)
        res = (SfAlignResult * G)()
        L = _abi.lib()
        L.sf_fuser_align_groups_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64,
                                                   C.c_void_p, C.POINTER(SfAlignParams), C.c_void_p, C.c_void_p]
        d_depth, d_rgb, rgb_stride = self._staged(depth), None, 0
        try:
            if rgb is not None:
                rgb = self._align_rgb(rgb, K)
                rgb_stride = rgb.size // K
                d_rgb = self._staged(rgb)
            check(L.sf_fuser_align_groups_device(self._h, d_depth, px * 2, d_rgb, rgb_stride, K, _ptr(members), _ptr(group_first), G, _ptr(poses), C.byref(a),
                                                 _ptr(out), C.cast(res, C.c_void_p)))
        finally:
            L.sf_device_free(d_depth)
            if d_rgb is not None:
                L.sf_device_free(d_rgb)
        return out, list(res)

    def align_scan(self, depth, poses, params=None, scan=None, rgb=None):
        """sf_fuser_align_scan: K u16 keyframes (host, [K, H*W]) of any number up to 4096 with camToWorld poses [K,16]: groups of consecutive keyframes
        under the global solve.  rgb: the keyframes' pictures (the colour term) -> (poses float32 [K,16], SfAlignScanResult)."""
        a = params if params is not None else default_align_params()
        sp = scan if scan is not None else default_align_scan_params()
        poses = np.ascontiguousarray(poses, dtype=np.float32).reshape(-1, 16)
        depth = np.ascontiguousarray(depth, dtype=np.uint16)
        if depth.size != len(poses) * self.params.depth_width * self.params.depth_height:
            raise ValueError("depth holds %d pixels, %d frames of %dx%d expected" % (depth.size, len(poses), self.params.depth_width, self.params.depth_height))
        if rgb is not None:
            rgb = self._align_rgb(rgb, len(poses))
        out = np.empty_like(poses)
        res = SfAlignScanResult()
        L = _abi.lib()
        L.sf_fuser_align_scan.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(SfAlignParams), C.POINTER(SfAlignScanParams),
                                          C.c_void_p, C.POINTER(SfAlignScanResult)]
        check(L.sf_fuser_align_scan(self._h, _ptr(depth), _ptr(rgb), len(poses), _ptr(poses), C.byref(a), C.byref(sp), _ptr(out), C.byref(res)))
        return out, res

    def align_scan_device(self, d_depth, frame_stride_bytes, poses, params=None, scan=None, d_rgb=None, rgb_stride_bytes=0):
        """align_scan() for keyframes already in HBM, `frame_stride_bytes` apart (sf_fuser_align_scan_device)."""
        a = params if params is not None else default_align_params()
        sp = scan if scan is not None else default_align_scan_params()
        poses = np.ascontiguousarray(poses, dtype=np.float32).reshape(-1, 16)
        out = np.empty_like(poses)
        res = SfAlignScanResult()
        L = _abi.lib()
        L.sf_fuser_align_scan_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.POINTER(SfAlignParams),
                                                 C.POINTER(SfAlignScanParams), C.c_void_p, C.POINTER(SfAlignScanResult)]
        check(L.sf_fuser_align_scan_device(self._h, _ptr(d_depth), int(frame_stride_bytes), _ptr(d_rgb), int(rgb_stride_bytes), len(poses), _ptr(poses),
                                           C.byref(a), C.byref(sp), _ptr(out), C.byref(res)))
        return out, res

    def align_groups_device(self, d_depth, frame_stride_bytes, K, members, group_first, poses, params=None, d_rgb=None, rgb_stride_bytes=0):
        """align_groups() for keyframes already in HBM."""
        a = params if params is not None else default_align_params()
        members = np.ascontiguousarray(members, dtype=np.int32).reshape(-1)
        group_first = np.ascontiguousarray(group_first, dtype=np.int32).reshape(-1)
        poses = np.ascontiguousarray(poses, dtype=np.float32).reshape(-1, 16)
        G = len(group_first) - 1
        out = np.empty_like(poses)
        res = (SfAlignResult * max(G, 1))()
        L = _abi.lib()
        L.sf_fuser_align_groups_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64,
                                                   C.c_void_p, C.POINTER(SfAlignParams), C.c_void_p, C.c_void_p]
        check(L.sf_fuser_align_groups_device(self._h, _ptr(d_depth), int(frame_stride_bytes), _ptr(d_rgb), int(rgb_stride_bytes), int(K), _ptr(members),
                                             _ptr(group_first), G, _ptr(poses), C.byref(a), _ptr(out), C.cast(res, C.c_void_p)))
        return out, list(res)

    def align_system(self, depth, poses, pairs, params=None):
        """Test hook (scanfuse_internal.h sf_fuser_align_system): the P per-pair 29-value systems (float64 [P,29]) at the given poses."""
        a, poses, pairs = self._align_args(poses, pairs, params)
        depth = np.ascontiguousarray(depth, dtype=np.uint16)
        sys = np.zeros((len(pairs), 29), np.float64)
        L = _abi.lib()
        L.sf_fuser_align_system.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(SfAlignParams), C.c_void_p]
        check(L.sf_fuser_align_system(self._h, _ptr(depth), len(poses), _ptr(poses), _ptr(pairs), len(pairs), C.byref(a), _ptr(sys)))
        return sys

    def align_rgbd_system(self, depth, rgb, poses, pairs, params=None):
        """Test hook (scanfuse_internal.h sf_fuser_align_rgbd_system): the P per-pair 31-value systems (float64 [P,31]) at the given poses; rgb may be
        None when colour_weight is 0."""
        a, poses, pairs = self._align_args(poses, pairs, params)
        depth = np.ascontiguousarray(depth, dtype=np.uint16)
        if rgb is not None:
            rgb = self._align_rgb(rgb, len(poses))
        sys = np.zeros((len(pairs), 31), np.float64)
        L = _abi.lib()
        L.sf_fuser_align_rgbd_system.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(SfAlignParams),
                                                 C.c_void_p]
        check(L.sf_fuser_align_rgbd_system(self._h, _ptr(depth), _ptr(rgb) if rgb is not None else None, len(poses), _ptr(poses), _ptr(pairs), len(pairs),
                                           C.byref(a), _ptr(sys)))
        return sys

    # -- camera tracking (DESIGN.md "Camera tracking" and "The colour term of the tracker") ---------------
    def _track_rgb(self, rgb):
        """The frame's RGB8 picture at the size the fuser fuses colour at."""
        rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
        w, h = (self.params.color_width, self.params.color_height) if self.params.color_width > 0 else (self.params.depth_width, self.params.depth_height)
        if rgb.size != w * h * 3:
            raise ValueError("picture has %d bytes, fuser expects %dx%dx3" % (rgb.size, w, h))
        return rgb

    def track(self, depth, guess, ref=None, params=None, rgb=None):
        """Track one u16 depth frame (host, the fuser's input size) against the volume, starting at camToWorld `guess`; the model is ray-cast at
        `ref` (None: the guess).  rgb: the frame's RGB8 picture (color_width x color_height, else the depth frames' own size): sf_fuser_track_rgbd, the
        colour term of DESIGN.md 4g with the parameters' colour_weight.  -> (pose float32 [4,4] or None when lost, SfTrackResult)."""
        t = params if params is not None else default_track_params()
        depth = np.ascontiguousarray(depth, dtype=np.uint16)
        if depth.size != self.params.depth_width * self.params.depth_height:
            raise ValueError("depth frame has %d pixels, fuser expects %dx%d" % (depth.size, self.params.depth_width, self.params.depth_height))
        if rgb is not None:
            return self._track(_abi.lib().sf_fuser_track_rgbd, _ptr(depth), guess, ref, t, (_ptr(self._track_rgb(rgb)),))
        return self._track(_abi.lib().sf_fuser_track, _ptr(depth), guess, ref, t)

    def track_device(self, d_depth, guess, ref=None, params=None, d_rgb=None):
        """track() for a u16 depth frame already in HBM (torch tensor or raw pointer), read on self.stream.  d_rgb: the frame's picture in HBM
        (sf_fuser_track_rgbd_device)."""
        t = params if params is not None else default_track_params()
        if d_rgb is not None:
            return self._track(_abi.lib().sf_fuser_track_rgbd_device, _ptr(d_depth), guess, ref, t, (_ptr(d_rgb),))
        return self._track(_abi.lib().sf_fuser_track_device, _ptr(d_depth), guess, ref, t)

    def _track(self, fn, depth_ptr, guess, ref, t, rgb_ptr=()):
        guess = np.ascontiguousarray(guess, dtype=np.float32).reshape(16)
        ref = None if ref is None else np.ascontiguousarray(ref, dtype=np.float32).reshape(16)
        out = np.empty(16, np.float32)
        res = SfTrackResult()
        fn.argtypes = [C.c_void_p, C.c_void_p] + [C.c_void_p] * len(rgb_ptr) + [C.c_void_p, C.c_void_p, C.POINTER(SfTrackParams), C.c_void_p, C.POINTER(SfTrackResult)]
        check(fn(self._h, depth_ptr, *rgb_ptr, _ptr(guess), _ptr(ref), C.byref(t), _ptr(out), C.byref(res)))
        return (out.reshape(4, 4) if res.tracked else None), res

    def track_system(self, depth, level, T, T_ref, params=None, mask=False, rgb=None, colour=False):
        """Test hook (scanfuse_internal.h sf_fuser_track_system): one level's 29-value system (float64) at estimate T with the model cast at
        T_ref, and the level's correspondence mask (u8 [H_l, W_l]) when mask=True.  rgb (or colour=True with rgb None, which needs colour_weight 0):
        sf_fuser_track_rgbd_system, the 31 values with the colour term."""
        t = params if params is not None else default_track_params()
        depth = np.ascontiguousarray(depth, dtype=np.uint16)
        T = np.ascontiguousarray(T, dtype=np.float32).reshape(16)
        T_ref = np.ascontiguousarray(T_ref, dtype=np.float32).reshape(16)
        colour = colour or rgb is not None
        sys = np.zeros(31 if colour else 29, np.float64)
        m = None
        if mask:
            W, H = self.raycast_size()
            m = np.zeros((H >> level, W >> level), np.uint8)
        L = _abi.lib()
        if colour:
            rgb = None if rgb is None else self._track_rgb(rgb)
            L.sf_fuser_track_rgbd_system.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(SfTrackParams), C.c_void_p,
                                                     C.c_void_p]
            check(L.sf_fuser_track_rgbd_system(self._h, _ptr(depth), _ptr(rgb), int(level), _ptr(T), _ptr(T_ref), C.byref(t), _ptr(sys), _ptr(m)))
        else:
            L.sf_fuser_track_system.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(SfTrackParams), C.c_void_p, C.c_void_p]
            check(L.sf_fuser_track_system(self._h, _ptr(depth), int(level), _ptr(T), _ptr(T_ref), C.byref(t), _ptr(sys), _ptr(m)))
        return (sys, m) if mask else sys

    def export_blocks(self):
        """-> (coords int32 [n,3], voxels VOXEL_DTYPE [n,512]) sorted lexicographically by (x,y,z)."""
        n = C.c_uint64(0)
        check(_abi.lib().sf_fuser_export_blocks(self._h, None, None, 0, C.byref(n)))
        coords = np.zeros((n.value, 3), np.int32)
        vox = np.zeros((n.value, 512), VOXEL_DTYPE)
        if n.value:
            check(_abi.lib().sf_fuser_export_blocks(self._h, _ptr(coords), _ptr(vox), n.value, C.byref(n)))
        order = np.lexsort((coords[:, 2], coords[:, 1], coords[:, 0]))
        return coords[order], vox[order]

    # -- the sparse volume as a dense one (scannet_amd/csrc/fuser_dense.hip) ------------------------------------------
    def allocate_box(self, lo_block, hi_block):
        """Insert every block of [lo_block, hi_block] (inclusive block coordinates) that the table does not hold, with zeroed voxels, on the
        device; blocks that exist keep their bytes.  Returns how many were new."""
        L = _abi.lib()
        lo = np.ascontiguousarray(lo_block, np.int32).reshape(3)
        hi = np.ascontiguousarray(hi_block, np.int32).reshape(3)
        n = C.c_uint64(0)
        check(L.sf_fuser_allocate_box(self._h, _ptr(lo), _ptr(hi), C.byref(n)))
        return n.value

    def known_bounds(self):
        """-> (lo int32 [3], hi int32 [3], known): the inclusive box, in global voxel indices, of the owned voxels with weight > 0 and their
        count; (None, None, 0) when there is none."""
        L = _abi.lib()
        lo, hi = np.zeros(3, np.int32), np.zeros(3, np.int32)
        n = C.c_uint64(0)
        check(L.sf_fuser_known_bounds(self._h, _ptr(lo), _ptr(hi), C.byref(n)))
        return (lo, hi, n.value) if n.value else (None, None, 0)

    def export_dense(self, lo, dims, task=False, rgb=False, device=False):
        """Region [lo, lo + dims) (global voxel indices, x y z) of the volume as dense [z][y][x] arrays -> (sdf float32, weight uint8) or, with
        rgb, (sdf, weight, rgb uint8 [..., 3]).  task: the task volume (-inf where weight == 0, else sdf / voxel_size) instead of sdf as stored.
        device: torch tensors on the fuser's GPU, written in place, instead of numpy arrays."""
        L = _abi.lib()
        lo = np.ascontiguousarray(lo, np.int32).reshape(3)
        dims = np.ascontiguousarray(dims, np.int32).reshape(3)
        if (dims <= 0).any():
            raise ValueError("dims must be positive")
        shape = (int(dims[2]), int(dims[1]), int(dims[0]))
        if device:
            import torch
            dev = torch.device("cuda", self.device)
            sdf = torch.empty(shape, dtype=torch.float32, device=dev)
            w = torch.empty(shape, dtype=torch.uint8, device=dev)
            c = torch.empty(shape + (3,), dtype=torch.uint8, device=dev) if rgb else None
            torch.cuda.synchronize(dev)
        else:
            sdf = np.empty(shape, np.float32)
            w = np.empty(shape, np.uint8)
            c = np.empty(shape + (3,), np.uint8) if rgb else None
        check(L.sf_fuser_export_dense(self._h, _ptr(lo), _ptr(dims), 1 if task else 0, _ptr(sdf), _ptr(w), _ptr(c), 1 if device else 0))
        return (sdf, w, c) if rgb else (sdf, w)

    # -- stage hooks of the front chain (scanfuse_internal.h sf_fuser_stage_*; tests/test_front_stages.py) ----------------------------------
    def _stage_sizes(self):
        p = self.params
        resampled = p.integration_width > 0 and p.integration_height > 0
        W, H = (p.integration_width, p.integration_height) if resampled else (p.depth_width, p.depth_height)
        return p.depth_width * p.depth_height, W * H

    def _stage_frames(self, depth, poses=None):
        depth = np.ascontiguousarray(depth, dtype=np.uint16)
        in_px, _ = self._stage_sizes()
        if depth.size == 0 or depth.size % in_px:
            raise ValueError("depth must hold whole frames of %d pixels" % in_px)
        n = depth.size // in_px
        if poses is not None:
            poses = np.ascontiguousarray(poses, dtype=np.float32).reshape(-1, 16)
            if len(poses) != n:
                raise ValueError("%d frames, %d poses" % (n, len(poses)))
        return depth, poses, n

    def stage_prepass(self, depth, rgb=None, misalign=0, jpeg=None):
        """k_prepass alone on n host frames: depthf float32 [n, W*H] and, with colour (rgb: n tight RGB8 pictures, the device copy `misalign` bytes past an
        aligned address; or jpeg: a list of n baseline streams), the texels uint64 [n, W*H] = depth bits | rgb << 32."""
        depth, _, n = self._stage_frames(depth)
        _, npx = self._stage_sizes()
        depthf = np.zeros((n, npx), np.float32)
        texel = np.zeros((n, npx), np.uint64) if (rgb is not None or jpeg is not None) else None
        streams = sizes = None
        if rgb is not None:
            rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
            p = self.params
            cw, ch = (p.color_width, p.color_height) if p.color_width > 0 and p.color_height > 0 else (p.depth_width, p.depth_height)
            if rgb.size != n * cw * ch * 3:
                raise ValueError("rgb must hold %d pictures of %dx%dx3" % (n, cw, ch))
        if jpeg is not None:
            keep = [np.frombuffer(bytes(b), np.uint8) for b in jpeg]
            streams = (C.c_void_p * len(keep))(*[b.ctypes.data for b in keep])
            sizes = (C.c_uint64 * len(keep))(*[b.size for b in keep])
            if len(keep) != n:
                raise ValueError("%d frames, %d pictures" % (n, len(keep)))
        L = _abi.lib()
        L.sf_fuser_stage_prepass.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        check(L.sf_fuser_stage_prepass(self._h, n, _ptr(depth), _ptr(rgb), int(misalign), streams, sizes, _ptr(depthf), _ptr(texel)))
        return depthf, texel

    def stage_alloc(self, depth, poses, head=False, fuse_pre=False, want_depth=False):
        """The front chain up to and including the allocation as one pass (seq0 = the fuser's next sequence number) -> dict(direct, probed, failed[, depthf])."""
        depth, poses, n = self._stage_frames(depth, poses)
        _, npx = self._stage_sizes()
        depthf = np.zeros((n, npx), np.float32) if want_depth else None
        d = (C.c_uint64 * 3)()
        L = _abi.lib()
        L.sf_fuser_stage_alloc.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        check(L.sf_fuser_stage_alloc(self._h, n, _ptr(depth), _ptr(poses), int(bool(head)), int(bool(fuse_pre)), _ptr(depthf), d))
        out = {"direct": int(d[0]), "probed": int(d[1]), "failed": int(d[2])}
        if want_depth:
            out["depthf"] = depthf
        return out

    def stage_compact(self, poses, seq0):
        """sf_launch_compact alone on the present directory -> dict(slots int32 [len], masks uint32 [len], length, last, total, tiles)."""
        poses = np.ascontiguousarray(poses, dtype=np.float32).reshape(-1, 16)
        cap = int(self.params.num_sdf_blocks)
        slots, masks = np.zeros(cap, np.int32), np.zeros(cap, np.uint32)
        word, d = C.c_uint64(0), (C.c_uint64 * 2)()
        L = _abi.lib()
        L.sf_fuser_stage_compact.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p]
        check(L.sf_fuser_stage_compact(self._h, len(poses), _ptr(poses), int(seq0), _ptr(slots), _ptr(masks), cap, C.byref(word), d))
        n = word.value & 0xFFFFFFFF
        return {"slots": slots[:n].copy(), "masks": masks[:n].copy(), "length": int(n), "last": int(word.value >> 32), "total": int(d[0]), "tiles": int(d[1])}

    def stage_live(self, include_ghosts=True):
        """sf_compact_live: the directory slots of every live block (or of those this fuser owns: include_ghosts False), int32."""
        cap = int(self.params.num_sdf_blocks)
        slots, n = np.zeros(cap, np.int32), C.c_uint64(0)
        L = _abi.lib()
        L.sf_fuser_stage_live.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        check(L.sf_fuser_stage_live(self._h, int(bool(include_ghosts)), _ptr(slots), cap, C.byref(n)))
        return slots[:n.value].copy()

    def stage_dump(self):
        """Host copies of the table (key, ptr, birth), heap, block_keys, block_entry, block_flags and the counter words."""
        p = self.params
        slots, nb = int(p.hash_num_buckets) * int(p.hash_bucket_size), int(p.num_sdf_blocks)
        out = {"key": np.zeros(slots, np.uint64), "ptr": np.zeros(slots, np.int32), "birth": np.zeros(slots, np.uint32), "heap": np.zeros(nb, np.int32),
               "block_keys": np.zeros(nb, np.uint64), "block_entry": np.zeros(nb, np.int32), "block_flags": np.zeros(nb, np.uint8), "counters": np.zeros(48, np.int32)}
        L = _abi.lib()
        L.sf_fuser_stage_dump.argtypes = [C.c_void_p] * 9
        check(L.sf_fuser_stage_dump(self._h, *[_ptr(out[k]) for k in ("key", "ptr", "birth", "heap", "block_keys", "block_entry", "block_flags", "counters")]))
        return out
