"""What an entry point answers when the device it is given cannot be opened (scannet_amd/csrc/hip_util.h open_device): the return code and the fragment
of sf_last_error that other tests and callers rely on, with no output handle made and no output array written.

One table drives both halves.  A row is (name, call, code past the end, fragment without a device); call(dev) -> (rc, untouched) runs the entry point with
arguments that pass every check ahead of the device and reports whether its outputs are as they were.

  * without a GPU (unmarked): device 0 gives SF_ERR_DEVICE and the row's fragment;
  * on the GPU (marked): device sf_device_count(), one past the end, gives the row's own code, and the process's current device stays what it was.

device = -1 (the host path where there is one, an error where there is not) is held by the tests of each module.

Left out, because something ahead of the device check cannot be satisfied in a line or two: sf_zlib_inflate_gpu (a fixed-Huffman stream that the device
takes), the three sf_simplify_stage_* hooks (a dozen output arrays each; sf_mesh_simplify_gpu opens its device the same way), sf_objvox_voxelize (a plan of
objects), sf_fuse_run_prepare (an open .sens file).

Then, on the GPU, two calls that cross functions whose call-local device buffers are scope-owned: the 256 weight records of sf_selftest_weight_records
against the statement of their four words, and sf_fuser_export_blocks_where of a one-block volume into host memory and into device memory, byte for byte.
"""
import ctypes as C

import numpy as np
import pytest

from scannet_amd import _abi

INVALID_ARG, DEVICE = -1, -5   # SF_ERR_INVALID_ARG, SF_ERR_DEVICE (include/scanfuse.h)
FILL = 7

XYZ = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)       # a tetrahedron: four vertices, four faces
TRIS = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], np.uint32)


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _handle(fn):
    """fn(pointer to a handle) -> (rc, the handle is still null)"""
    h = C.c_void_p()
    rc = fn(C.byref(h))
    return rc, not h.value


def _filled(shape, dtype):
    return np.full(shape, FILL, dtype)


def _same(*arrays):
    return all((a == FILL).all() for a in arrays)


def _mesh():
    from scannet_amd.segmentator import Mesh
    return Mesh.from_arrays(XYZ, TRIS)


def fuser_create(dev):
    p = _abi.SfParams()
    L = _abi.lib()
    L.sf_params_default(C.byref(p))
    return _handle(lambda h: L.sf_fuser_create(C.byref(p), dev, h))


def _jpeg(name):
    def call(dev):
        from scannet_amd import calibrate
        blob, out = np.zeros(64, np.uint8), _filled(16 * 16 * 3, np.uint8)   # the device is opened before the stream is parsed
        return getattr(calibrate._lib(), name)(_vp(blob), blob.size, 16, 16, dev, _vp(out)), _same(out)
    return call


def filter2d_create(dev):
    from scannet_amd import filter2d
    return _handle(lambda h: filter2d._lib().sf_filter2d_create(8, 8, 8, 8, dev, h))


def filter2d_stage_to_label(dev):
    from scannet_amd import filter2d
    inst, table, out = np.zeros(16, np.uint8), np.zeros(256, np.uint16), _filled(16, np.uint16)
    return filter2d._stage_lib().sf_filter2d_stage_to_label(dev, _vp(inst), _vp(table), 16, _vp(out)), _same(out)


def projector_create(dev):
    from scannet_amd import project
    p = project.default_params((16, 16), (16, 16), 10.0, 10.0)
    return _handle(lambda h: project._lib().sf_projector_create(C.byref(p), dev, h))


def calibrator_create(dev):
    from scannet_amd import calibrate
    K = (10.0, 10.0, 8.0, 8.0)
    p = calibrate.make_params((16, 16), (16, 16), K, K)
    return _handle(lambda h: calibrate._lib().sf_calibrator_create(C.byref(p), None, 1000.0, dev, h))


def mesh_simplify_gpu(dev):
    from scannet_amd import meshclean
    m = _mesh()
    p = meshclean.SfSimplifyParams()
    L = meshclean._lib()
    L.sf_simplify_default_params(C.byref(p))
    L.sf_mesh_simplify_gpu.argtypes = [C.c_void_p, C.POINTER(meshclean.SfSimplifyParams), C.c_int, C.POINTER(C.c_void_p), C.POINTER(meshclean.SfSimplifyStats)]
    return _handle(lambda h: L.sf_mesh_simplify_gpu(m._h, C.byref(p), dev, h, None))


def mesh_clean_gpu(dev):
    m = _mesh()
    L = _abi.lib()
    from scannet_amd import meshclean
    L.sf_mesh_clean_gpu.argtypes = [C.c_void_p, C.c_float, C.c_uint32, C.c_int, C.POINTER(C.c_void_p), C.POINTER(meshclean.SfCleanStats)]
    return _handle(lambda h: L.sf_mesh_clean_gpu(m._h, 0.0, 1, dev, h, None))


def clean_stage_components(dev):
    L = _abi.lib()
    L.sf_clean_stage_components.argtypes = [C.c_int, C.c_uint32] + [C.c_void_p, C.c_uint32] + [C.c_void_p] * 4
    root, size, keep, cnt = _filled(4, np.uint32), _filled(4, np.uint32), _filled(4, np.uint8), _filled(3, np.uint32)
    return L.sf_clean_stage_components(dev, 4, _vp(TRIS), 1, _vp(root), _vp(size), _vp(keep), _vp(cnt)), _same(root, size, keep, cnt)


def segment_mesh_gpu(dev):
    L = _abi.lib()
    L.sf_segment_mesh_gpu.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_float, C.c_int, C.c_int, C.c_void_p]
    out = _filled(4, np.int32)
    return L.sf_segment_mesh_gpu(_vp(XYZ), 4, _vp(TRIS), 4, 0.01, 1, dev, _vp(out)), _same(out)


def renderer_create(dev):
    from scannet_amd import render
    return _handle(lambda h: render._lib().sf_renderer_create(None, dev, h))


def lut_estimator_create(dev):
    from scannet_amd import depth_lut
    return _handle(lambda h: depth_lut._lib().sf_lut_estimator_create(16, 16, 10.0, 10.0, 8.0, 8.0, 4, 5.0, 1, dev, h))


def lut_apply(dev):
    from scannet_amd import depth_lut
    s, keep = depth_lut._lut_struct((np.ones((2, 2, 2), np.float32), 5.0))
    src, out = np.zeros((16, 16), np.uint16), _filled((16, 16), np.uint16)
    ip, op = (C.c_void_p * 1)(src.ctypes.data), (C.c_void_p * 1)(out.ctypes.data)
    return depth_lut._lib().sf_lut_apply(C.byref(s), 1, ip, op, 16, 16, 1, dev), _same(out) and keep is not None


def eval_confusion(dev):
    from scannet_amd import evaluation
    gt, pred, valid = np.ones(32, np.uint8), np.ones(32, np.uint8), np.array([1, 2], np.int32)
    table, oor = _filled(64 * 64, np.uint64), _filled(1, np.uint64)
    rc = evaluation._lib().sf_eval_confusion(_vp(gt), _vp(pred), 1, 32, _vp(valid), 2, evaluation.MODE_3D, dev, _vp(table), _vp(oor))
    return rc, _same(table, oor)


def voxlabel_nearest_faces(dev):
    from scannet_amd import voxel_labels as vl
    h = vl.header((4, 4, 4), 0.25, (0, 0, 0))
    face, d2 = _filled((4, 4, 4), np.int32), _filled((4, 4, 4), np.float32)
    rc = vl._lib().sf_voxlabel_nearest_faces(C.byref(h), _vp(XYZ), 4, _vp(TRIS), 4, 0.5, dev, _vp(face), _vp(d2))
    return rc, _same(face, d2)


def axis_align_stage_normals(dev):
    L = _abi.lib()
    L.sf_axis_align_stage_normals.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p]
    out = _filled((4, 3), np.float32)
    return L.sf_axis_align_stage_normals(_vp(XYZ), 4, _vp(TRIS), 4, dev, _vp(out)), _same(out)


# name, call, the code of a device index one past the end, the fragment without any device
ROWS = [
    ("sf_fuser_create", fuser_create, INVALID_ARG, b"no CPU fallback"),
    ("sf_jpeg_decode_gpu", _jpeg("sf_jpeg_decode_gpu"), INVALID_ARG, b"no CPU fallback"),
    ("sf_jpeg_decode_gpu_huffman", _jpeg("sf_jpeg_decode_gpu_huffman"), INVALID_ARG, b"no HIP device"),
    ("sf_filter2d_create", filter2d_create, INVALID_ARG, b"no CPU fallback"),
    ("sf_filter2d_stage_to_label", filter2d_stage_to_label, INVALID_ARG, b"no CPU fallback"),
    ("sf_projector_create", projector_create, INVALID_ARG, b"no CPU fallback"),
    ("sf_calibrator_create", calibrator_create, INVALID_ARG, b"no CPU fallback"),
    ("sf_mesh_simplify_gpu", mesh_simplify_gpu, INVALID_ARG, b"no HIP device"),
    ("sf_mesh_clean_gpu", mesh_clean_gpu, INVALID_ARG, b"no HIP device"),
    ("sf_clean_stage_components", clean_stage_components, INVALID_ARG, b"no HIP device"),
    ("sf_segment_mesh_gpu", segment_mesh_gpu, INVALID_ARG, b"no HIP device"),
    ("sf_renderer_create", renderer_create, DEVICE, b"never taken silently"),
    ("sf_lut_estimator_create", lut_estimator_create, INVALID_ARG, b"no HIP device"),
    ("sf_lut_apply", lut_apply, INVALID_ARG, b"no HIP device"),
    ("sf_eval_confusion", eval_confusion, DEVICE, b"no HIP device"),
    ("sf_voxlabel_nearest_faces", voxlabel_nearest_faces, DEVICE, b"no HIP device"),
    ("sf_axis_align_stage_normals", axis_align_stage_normals, INVALID_ARG, b"no HIP device"),
]
IDS = [r[0] for r in ROWS]


@pytest.mark.parametrize("name,call,code,fragment", ROWS, ids=IDS)
def test_without_a_device(name, call, code, fragment):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    rc, untouched = call(0)
    msg = _abi.lib().sf_last_error()
    print(name, rc, msg)
    assert rc == DEVICE and fragment in msg and untouched


def _drain_last_error():
    """A refused create may destroy its half-built object on the device it was refused (sf_renderer_create, sf_lut_estimator_create), which leaves the
    runtime's last error set on this thread; the next launch check of anybody -- this library's or torch's -- would report it.  Read it away."""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            hip = C.CDLL(line.split()[-1])          # the runtime this process already holds
            hip.hipGetLastError()
            return


@pytest.mark.gpu
@pytest.mark.parametrize("name,call,code,fragment", ROWS, ids=IDS)
def test_one_past_the_last_device(name, call, code, fragment):
    import torch
    L = _abi.lib()
    n = C.c_int(-1)
    assert L.sf_device_count(C.byref(n)) == 0 and n.value >= 1
    before = torch.cuda.current_device()          # hipGetDevice of the runtime the library shares with torch
    rc, untouched = call(n.value)
    msg = L.sf_last_error()
    _drain_last_error()
    print(name, rc, msg)
    assert rc == code and msg and untouched
    assert torch.cuda.current_device() == before


@pytest.mark.gpu
def test_weight_records_cross_a_scope_owned_buffer():
    L = _abi.lib()
    L.sf_selftest_weight_records.argtypes = [C.c_int, C.c_void_p]
    out = np.zeros((256, 4), np.uint32)
    _abi.check(L.sf_selftest_weight_records(0, _vp(out)))
    w = np.arange(256, dtype=np.uint32)                       # fuser_internal.h fill_weight_records: (float)w, (float)(w + 1), 1 / (w + 1), the weight word
    want = np.zeros((256, 4), np.uint32)
    want[:, 0] = w.astype(np.float32).view(np.uint32)
    want[:, 1] = (w + 1).astype(np.float32).view(np.uint32)
    want[:, 2] = (np.float32(1) / (w + 1).astype(np.float32)).view(np.uint32)
    want[:, 3] = (np.minimum(w + 1, 255) << 24) | np.where(w == 0, 0x00FFFFFF, 0).astype(np.uint32)
    assert np.array_equal(out, want)


@pytest.mark.gpu
def test_export_where_to_host_and_to_device_memory_agree():
    import torch
    from scannet_amd import fusion
    L = _abi.lib()
    with fusion.Fuser(fusion.default_params(depth_width=64, depth_height=48, num_sdf_blocks=1 << 10, hash_num_buckets=1 << 10), device=0) as f:
        assert f.allocate_box((3, -2, 5), (3, -2, 5)) == 1
        n = C.c_uint64(0)
        hc, hv = _filled((2, 3), np.int32), _filled((2, 4096), np.uint8)          # room for two: the second block's bytes stay as they were
        _abi.check(L.sf_fuser_export_blocks_where(f._h, 0, 3, 4, 0, _vp(hc), _vp(hv), 2, C.byref(n), 0))
        assert n.value == 1 and hc[0].tolist() == [3, -2, 5] and not hv[0].any() and _same(hc[1], hv[1])
        dc = torch.full((2, 3), FILL, dtype=torch.int32, device="cuda:0")
        dv = torch.full((2, 4096), FILL, dtype=torch.uint8, device="cuda:0")
        _abi.check(L.sf_fuser_export_blocks_where(f._h, 0, 3, 4, 0, C.c_void_p(dc.data_ptr()), C.c_void_p(dv.data_ptr()), 2, C.byref(n), 1))
        assert n.value == 1
        assert dc.cpu().numpy().tobytes() == hc.tobytes() and dv.cpu().numpy().tobytes() == hv.tobytes()
        _abi.check(L.sf_fuser_export_blocks_where(f._h, 0, 4, 9, 0, _vp(hc), _vp(hv), 2, C.byref(n), 0))    # a slab without blocks: nothing written
        assert n.value == 0 and hc[0].tolist() == [3, -2, 5] and _same(hc[1], hv[1])
