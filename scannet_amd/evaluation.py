"""The benchmark's scores from predictions: the label confusion matrix and IoU (3-D and 2-D), and the instance AP, over the C ABI (include/scanfuse.h
"Benchmark scores"; scannet_amd/csrc/evaluation.cpp, evaluation.hip; the rules are DESIGN.md section 4o).  What they replace in the reference tree:
BenchmarkScripts/3d_evaluation/evaluate_semantic_label.py, evaluate_semantic_instance.py with util_3d.py, and
2d_evaluation/evalPixelLevelSemanticLabeling.py, and 3d_helpers/export_train_mesh_for_evaluation.py (export_ground_truth); and the 2-D instance AP
(scannet_amd/csrc/instance2d.cpp, instance2d_files.cpp): 2d_evaluation/evalInstanceLevelSemanticLabeling.py with
instances2dict.py and instance.py.

The array functions take numpy arrays or torch tensors on `cuda:N`.  numpy: `device=None` is the host path (at most 16 threads), an int copies to that
GPU and runs the kernels; the counts are the same.  Tensors on a GPU go to the `_device` entry points on torch's current stream: nothing is copied to
the host, nothing waits, and the result stays a device tensor until `.numpy()` asks for it."""
import ctypes as C
import os

import numpy as np

from . import _abi
from ._abi import check

# evaluate_semantic_label.py:43-44 and evaluate_semantic_instance.py:57-58
LABEL_NAMES = ("wall", "floor", "cabinet", "bed", "chair", "sofa", "table", "door", "window", "bookshelf", "picture", "counter", "desk", "curtain", "refrigerator",
               "shower curtain", "toilet", "sink", "bathtub", "otherfurniture")
LABEL_IDS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39)
INSTANCE_NAMES = LABEL_NAMES[2:]
INSTANCE_IDS = LABEL_IDS[2:]
MODE_3D, MODE_2D = 0, 1
IMAGE_WIDTH, IMAGE_HEIGHT = 640, 480
AP_OVERLAPS = 10


def _lib():
    L = _abi.lib()
    vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
    L.sf_eval_confusion.argtypes = [vp, vp, i32, u64, vp, u32, i32, i32, vp, vp]
    L.sf_eval_confusion_device.argtypes = [vp, vp, i32, u64, vp, u32, i32, vp, vp, vp]
    L.sf_eval_confusion_images.argtypes = [vp, vp, i32, u32, u32, u32, u32, u32, u32, i32, vp, vp]
    L.sf_eval_confusion_images_device.argtypes = [vp, vp, i32, u32, u32, u32, u32, u32, u32, vp, vp, vp]
    L.sf_eval_iou.argtypes = [vp, u32, vp, u32, vp, vp, vp]
    L.sf_eval_instance_plan.argtypes = [vp, u64, vp, u32, vp, vp, u32, vp, C.POINTER(u32)]
    L.sf_eval_instance_overlaps.argtypes = [vp, u64, u32, vp, u32, u64, i32, vp]
    L.sf_eval_instance_overlaps_device.argtypes = [vp, u64, u32, vp, u32, u64, vp, vp]
    L.sf_eval_ap_create.argtypes = [vp, u32, u32, C.POINTER(vp)]
    L.sf_eval_ap_add_scan.argtypes = [vp, u32, vp, vp, u32, vp, vp, vp]
    L.sf_eval_ap_finish.argtypes = [vp, vp, vp, vp]
    L.sf_eval_ap_destroy.argtypes = [vp]
    L.sf_eval_ap_destroy.restype = None
    L.sf_eval_ap_thresholds.argtypes = [vp]   # include/scanfuse_internal.h
    L.sf_eval_label_dir.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, i32, C.POINTER(vp)]
    L.sf_eval_instance_dir.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, u32, i32, C.POINTER(vp)]
    L.sf_eval_pixel_dir.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, i32, C.POINTER(vp)]
    L.sf_eval_image_plan.argtypes = [vp, i32, u32, u32, u32, vp, u32, u32, i32, vp, vp, vp]
    L.sf_eval_image_plan_scratch.argtypes = [u32, vp, u32]
    L.sf_eval_image_plan_scratch.restype = u64
    L.sf_eval_image_plan_device.argtypes = [vp, i32, u32, u32, u32, vp, u32, u32, vp, vp, vp, vp, vp]
    L.sf_eval_overlaps_images.argtypes = [vp, i32, u32, u32, u32, vp, u32, u32, vp, vp, vp, u32, u64, vp, i32, vp]
    L.sf_eval_overlaps_images_device.argtypes = [vp, i32, u32, u32, u32, vp, u32, u32, vp, vp, vp, u32, u64, vp, vp, vp]
    L.sf_eval_ap2d_create.argtypes = [vp, u32, u32, C.POINTER(vp)]
    L.sf_eval_ap2d_add_image.argtypes = [vp, u32, vp, vp, u32, vp, vp, vp, u32]
    L.sf_eval_ap2d_finish.argtypes = [vp, vp, vp, vp]
    L.sf_eval_ap2d_destroy.argtypes = [vp]
    L.sf_eval_ap2d_destroy.restype = None
    L.sf_eval_ap2d_thresholds.argtypes = [vp]
    L.sf_eval_instance2d_dir.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, u32, i32, C.POINTER(vp)]
    L.sf_eval_export_ids.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, u64, vp, vp, C.POINTER(u64)]
    L.sf_eval_export_scan.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p]
    L.sf_free.argtypes = [vp]
    L.sf_free.restype = None
    return L


def _ptr(a):
    if a is None:
        return None
    if hasattr(a, "data_ptr"):
        return C.c_void_p(a.data_ptr())
    return a.ctypes.data_as(C.c_void_p)


def _is_tensor(a):
    return hasattr(a, "data_ptr") and hasattr(a, "is_cuda")


def _valid(valid_ids):
    v = np.ascontiguousarray(valid_ids, np.int32).reshape(-1)
    if len(v) == 0:
        raise ValueError("no valid class ids")
    return v


def dim_of(valid_ids):
    """Rows of the confusion matrix: the largest valid id + 2 (41 for NYU40's 20 classes)."""
    return int(max(valid_ids)) + 2


_UNSIGNED = {1: np.uint8, 2: np.uint16, 4: np.uint32}


def _np_elements(a, width):
    """An integer array as unsigned elements of `width` bytes.  A value that does not fit -- negative, or too large -- becomes the largest value, which
    is no class id and at least every dim."""
    a = np.asarray(a)
    if a.dtype == np.bool_:
        a = a.view(np.uint8)
    if a.dtype.kind not in "iu":
        raise TypeError("ids must be integers, not %s" % a.dtype)
    if a.dtype.itemsize == width:
        return np.ascontiguousarray(a).view(_UNSIGNED[width])
    top = np.iinfo(_UNSIGNED[width]).max
    out = np.full(a.shape, top, _UNSIGNED[width])
    fits = (a >= 0) & (a <= top) if a.dtype.kind == "i" else a <= top
    out[fits] = a[fits]
    return out


def _width(a, b):
    return min(4, max(np.asarray(a).dtype.itemsize, np.asarray(b).dtype.itemsize))


def _torch_elements(t, width):
    import torch
    if t.dtype == torch.bool:
        t = t.view(torch.uint8)
    if t.dtype.is_floating_point or t.dtype.is_complex:
        raise TypeError("ids must be integers, not %s" % t.dtype)
    if t.element_size() != width:
        signed = {1: torch.int8, 2: torch.int16, 4: torch.int32}[width]
        if t.element_size() > width:
            top = (1 << (8 * width - 1)) - 1
            t = torch.where((t < 0) | (t > top), torch.full_like(t, -1), t)   # no class either way
        t = t.to(signed)
    return t.contiguous()


class Counts:
    """A confusion matrix that can be added to: `matrix` [dim, dim] and `out_of_range` [1], numpy uint64 or torch int64 on the device of the call."""

    def __init__(self, dim, like=None):
        self.dim = int(dim)
        cells = self.dim * self.dim + 1
        if like is not None and _is_tensor(like):
            import torch
            self._flat = torch.zeros(cells, dtype=torch.int64, device=like.device)
        else:
            self._flat = np.zeros(cells, np.uint64)
        self.matrix = self._flat[:cells - 1].reshape(self.dim, self.dim)
        self.out_of_range = self._flat[cells - 1:]

    @property
    def on_device(self):
        return _is_tensor(self._flat)

    def numpy(self):
        """-> (matrix uint64 [dim, dim], out_of_range int): reads a device result back, which waits for it."""
        flat = self._flat.cpu().numpy().view(np.uint64) if self.on_device else self._flat
        return flat[:-1].reshape(self.dim, self.dim).copy(), int(flat[-1])


def _stream(t):
    import torch
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _pair(gt, pred, into, dim):
    """-> (gt, pred, width, tensors?, into)"""
    tensors = _is_tensor(gt) or _is_tensor(pred)
    if tensors:
        if not (_is_tensor(gt) and _is_tensor(pred) and gt.is_cuda and pred.is_cuda and gt.device == pred.device):
            raise ValueError("both arrays must be tensors on one GPU (or both numpy arrays)")
        width = min(4, max(gt.element_size(), pred.element_size()))
        gt, pred = _torch_elements(gt, width), _torch_elements(pred, width)
    else:
        width = _width(gt, pred)
        gt, pred = _np_elements(gt, width), _np_elements(pred, width)
    if into is None:
        into = Counts(dim, like=gt if tensors else None)
    elif into.dim != dim or into.on_device != tensors:
        raise ValueError("`into` holds a matrix of %d rows %s" % (into.dim, "on a device" if into.on_device else "on the host"))
    return gt, pred, width, tensors, into


def confusion(gt, pred, valid_ids=LABEL_IDS, mode=MODE_3D, device=None, into=None):
    """sf_eval_confusion / sf_eval_confusion_device -> Counts.  gt, pred: integer arrays of one shape.  mode MODE_3D: an element whose gt is no valid
    class is skipped, a pred that is no valid class counts in column dim - 1; MODE_2D: every element counts, ids >= dim go to out_of_range.
    into: a Counts of an earlier call to add to."""
    L = _lib()
    v = _valid(valid_ids)
    if tuple(gt.shape) != tuple(pred.shape):
        raise ValueError("%s predictions for %s ground-truth values" % (tuple(pred.shape), tuple(gt.shape)))
    gt, pred, width, tensors, into = _pair(gt, pred, into, dim_of(v))
    n = int(gt.numel()) if tensors else int(gt.size)
    if tensors:
        check(L.sf_eval_confusion_device(_ptr(gt), _ptr(pred), width, n, _ptr(v), len(v), int(mode), _stream(gt), _ptr(into.matrix), _ptr(into.out_of_range)))
    else:
        check(L.sf_eval_confusion(_ptr(gt), _ptr(pred), width, n, _ptr(v), len(v), int(mode), -1 if device is None else int(device), _ptr(into.matrix),
                                  _ptr(into.out_of_range)))
    return into


def confusion_images(gt, pred, dim=41, device=None, into=None):
    """sf_eval_confusion_images(_device) -> Counts.  gt [B, H, W] (or [H, W]) and pred [B, h, w]: both are resized to 640 x 480 by nearest neighbour
    inside the call and counted in the 2-D mode.  The prediction has the ground truth's width or is 640 x 480."""
    L = _lib()
    if gt.ndim == 2:
        gt, pred = gt[None], pred[None]
    if gt.ndim != 3 or pred.ndim != 3 or gt.shape[0] != pred.shape[0]:
        raise ValueError("image batches of shapes %s and %s" % (tuple(gt.shape), tuple(pred.shape)))
    gt, pred, width, tensors, into = _pair(gt, pred, into, int(dim))
    sizes = (int(gt.shape[0]), int(gt.shape[2]), int(gt.shape[1]), int(pred.shape[2]), int(pred.shape[1]), int(dim))
    if tensors:
        check(L.sf_eval_confusion_images_device(_ptr(gt), _ptr(pred), width, *sizes, _stream(gt), _ptr(into.matrix), _ptr(into.out_of_range)))
    else:
        check(L.sf_eval_confusion_images(_ptr(gt), _ptr(pred), width, *sizes, -1 if device is None else int(device), _ptr(into.matrix), _ptr(into.out_of_range)))
    return into


def iou(matrix, valid_ids=LABEL_IDS):
    """sf_eval_iou -> (iou float64 [n_valid], NaN where the denominator is 0; tp uint64 [n_valid]; denom uint64 [n_valid]).  matrix: a Counts or an
    array [dim, dim]."""
    if isinstance(matrix, Counts):
        matrix = matrix.numpy()[0]
    m = np.ascontiguousarray(matrix, np.uint64)
    if m.ndim != 2 or m.shape[0] != m.shape[1]:
        raise ValueError("a square matrix")
    v = _valid(valid_ids)
    out, tp, denom = np.zeros(len(v), np.float64), np.zeros(len(v), np.uint64), np.zeros(len(v), np.uint64)
    check(_lib().sf_eval_iou(_ptr(m), m.shape[0], _ptr(v), len(v), _ptr(out), _ptr(tp), _ptr(denom)))
    return out, tp, denom


def instance_plan(gt_ids, valid_ids=INSTANCE_IDS):
    """sf_eval_instance_plan -> (instance_id int32 [G] ascending, instance_verts uint32 [G], slot uint32 [n]: the instance of every vertex, G = void)."""
    L = _lib()
    ids = np.ascontiguousarray(gt_ids, np.int32).reshape(-1)
    v = _valid(valid_ids)
    count = C.c_uint32(0)
    slot = np.zeros(len(ids), np.uint32)
    check(L.sf_eval_instance_plan(_ptr(ids), len(ids), _ptr(v), len(v), None, None, 0, _ptr(slot), C.byref(count)))
    G = count.value
    iid, verts = np.zeros(G, np.int32), np.zeros(G, np.uint32)
    check(L.sf_eval_instance_plan(_ptr(ids), len(ids), _ptr(v), len(v), _ptr(iid), _ptr(verts), G, None, C.byref(count)))
    return iid, verts, slot


def instance_overlaps(slot, G, masks, device=None):
    """sf_eval_instance_overlaps(_device) -> table uint32 [P, G + 2] (torch: int32 on the device): per prediction the covered vertices in each
    instance, in void, and in all.  slot [n] (instance_plan's); masks [P, n] of bytes or bools, rows may be further apart than n."""
    L = _lib()
    G = int(G)
    if _is_tensor(masks) or _is_tensor(slot):
        import torch
        if not (_is_tensor(masks) and _is_tensor(slot) and masks.is_cuda and slot.device == masks.device):
            raise ValueError("slot and masks must be tensors on one GPU (or both numpy arrays)")
        if masks.dtype == torch.bool:
            masks = masks.view(torch.uint8)
        if masks.element_size() != 1 or slot.element_size() != 4 or slot.dtype.is_floating_point:
            raise TypeError("masks of bytes and slots of 32-bit integers")
        if masks.ndim != 2 or (masks.shape[0] > 1 and masks.shape[1] > 1 and masks.stride(1) != 1) or (masks.shape[0] > 1 and masks.stride(0) < masks.shape[1]):
            masks = masks.contiguous()
        slot = slot.contiguous()
        P, n = int(masks.shape[0]), int(masks.shape[1])
        if n != slot.numel():
            raise ValueError("masks over %d vertices, slots for %d" % (n, slot.numel()))
        stride = int(masks.stride(0)) if P > 1 else n
        table = torch.zeros((P, G + 2), dtype=torch.int32, device=masks.device)
        check(L.sf_eval_instance_overlaps_device(_ptr(slot), n, G, _ptr(masks), P, stride, _stream(masks), _ptr(table)))
        return table
    masks = np.asarray(masks)
    if masks.dtype == np.bool_:
        masks = masks.view(np.uint8)
    if masks.dtype.itemsize != 1:
        raise TypeError("masks of bytes")
    slot = np.ascontiguousarray(slot, np.uint32).reshape(-1)
    if masks.ndim != 2 or masks.shape[1] != len(slot):
        raise ValueError("masks %s over %d vertices" % (masks.shape, len(slot)))
    P, n = masks.shape
    if P > 1 and n > 0 and (masks.strides[1] != 1 or masks.strides[0] < n):
        masks = np.ascontiguousarray(masks)
    stride = int(masks.strides[0]) if P > 1 and n > 0 else n
    table = np.zeros((P, G + 2), np.uint32)
    check(L.sf_eval_instance_overlaps(_ptr(slot), n, G, _ptr(masks), P, stride, -1 if device is None else int(device), _ptr(table)))
    return table


def ap_thresholds():
    """The overlap thresholds of the AP, bit for bit (sf_eval_ap_thresholds)."""
    th = np.zeros(AP_OVERLAPS, np.float64)
    check(_lib().sf_eval_ap_thresholds(_ptr(th)))
    return th


class InstanceAP:
    """The AP over scans (sf_eval_ap_*).  add(): a scan from its ground-truth ids and prediction masks; add_scan(): from a plan and an overlap table;
    finish() -> {"ap": [n_valid, 10], "classes": {name: {"ap", "ap50%", "ap25%"}}, "all_ap", "all_ap_50%", "all_ap_25%"}."""

    def __init__(self, valid_ids=INSTANCE_IDS, names=INSTANCE_NAMES, min_region_size=100):
        self._L = _lib()
        self.valid_ids = _valid(valid_ids)
        self.names = tuple(names)
        if len(self.names) != len(self.valid_ids):
            raise ValueError("one name per valid class id")
        self._h = C.c_void_p()
        check(self._L.sf_eval_ap_create(_ptr(self.valid_ids), len(self.valid_ids), int(min_region_size), C.byref(self._h)))

    def close(self):
        if self._h.value:
            self._L.sf_eval_ap_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def add_scan(self, instance_id, instance_verts, pred_label, pred_conf, table):
        if _is_tensor(table):
            table = table.cpu().numpy()
        iid = np.ascontiguousarray(instance_id, np.int32).reshape(-1)
        verts = np.ascontiguousarray(instance_verts, np.uint32).reshape(-1)
        label = np.ascontiguousarray(pred_label, np.int32).reshape(-1)
        conf = np.ascontiguousarray(pred_conf, np.float64).reshape(-1)
        table = np.ascontiguousarray(table).view(np.uint32) if np.asarray(table).dtype.itemsize == 4 else np.ascontiguousarray(table, np.uint32)
        G, P = len(iid), len(label)
        if len(verts) != G or len(conf) != P or table.shape != (P, G + 2):
            raise ValueError("a table of %s for %d predictions and %d instances" % (table.shape, P, G))
        check(self._L.sf_eval_ap_add_scan(self._h, G, _ptr(iid), _ptr(verts), P, _ptr(label), _ptr(conf), _ptr(table)))

    def add(self, gt_ids, masks, pred_label, pred_conf, device=None):
        """gt_ids [n] (numpy, label * 1000 + k); masks [P, n]: numpy, or a tensor on a GPU (the slots are sent there, the masks stay)."""
        iid, verts, slot = instance_plan(gt_ids, self.valid_ids)
        if _is_tensor(masks):
            import torch
            slot = torch.from_numpy(slot.view(np.int32)).to(masks.device)
        self.add_scan(iid, verts, pred_label, pred_conf, instance_overlaps(slot, len(iid), masks, device))

    def finish(self):
        n = len(self.valid_ids)
        ap, cls, avg = np.zeros((n, AP_OVERLAPS), np.float64), np.zeros((n, 3), np.float64), np.zeros(3, np.float64)
        check(self._L.sf_eval_ap_finish(self._h, _ptr(ap), _ptr(cls), _ptr(avg)))
        classes = {name: {"ap": cls[i, 0], "ap50%": cls[i, 1], "ap25%": cls[i, 2]} for i, name in enumerate(self.names)}
        return {"ap": ap, "classes": classes, "all_ap": avg[0], "all_ap_50%": avg[1], "all_ap_25%": avg[2]}


# ---- 2-D instances: the image-level instance AP ----

AP2D_OVERLAPS = 10


def _images(gt):
    """-> (images [B, H, W] contiguous, unsigned pixels of 1, 2 or 4 bytes; width in bytes; tensors?)"""
    if _is_tensor(gt):
        if not gt.is_cuda:
            raise ValueError("a tensor on a GPU (or a numpy array)")
        if gt.ndim == 2:
            gt = gt[None]
        width = min(4, gt.element_size())
        gt = _torch_elements(gt, width)
        tensors = True
    else:
        gt = np.asarray(gt)
        if gt.ndim == 2:
            gt = gt[None]
        width = min(4, gt.dtype.itemsize)
        gt = _np_elements(gt, width)
        tensors = False
    if gt.ndim != 3:
        raise ValueError("id images [B, H, W], not %s" % (tuple(gt.shape),))
    return gt, width, tensors


def image_plan(gt, valid_ids=INSTANCE_IDS, capacity=None, device=None):
    """sf_eval_image_plan(_device) -> (count uint32 [B], instance_id int32 [B, capacity] ascending, instance_pixels uint32 [B, capacity]); torch: int32
    tensors on the device.  gt [B, H, W] (or [H, W]): id images, a pixel is label * 1000 + k.  capacity None (numpy): the largest count of the batch;
    tensors need a capacity (the counts stay on the device); count[b] > capacity there means image b has more instances than were written."""
    L = _lib()
    v = _valid(valid_ids)
    gt, width, tensors = _images(gt)
    B, H, W = (int(x) for x in gt.shape)
    if tensors:
        import torch
        if capacity is None:
            raise ValueError("tensors need a capacity: the counts stay on the device")
        capacity = int(capacity)
        scratch = torch.empty(max(1, int(L.sf_eval_image_plan_scratch(B, _ptr(v), len(v))) // 4), dtype=torch.int32, device=gt.device)
        count = torch.zeros(B, dtype=torch.int32, device=gt.device)
        iid = torch.zeros((B, capacity), dtype=torch.int32, device=gt.device)
        px = torch.zeros((B, capacity), dtype=torch.int32, device=gt.device)
        check(L.sf_eval_image_plan_device(_ptr(gt), width, B, W, H, _ptr(v), len(v), capacity, _stream(gt), _ptr(scratch), _ptr(count), _ptr(iid), _ptr(px)))
        scratch.record_stream(torch.cuda.current_stream(gt.device))
        return count, iid, px
    dev = -1 if device is None else int(device)
    count = np.zeros(B, np.uint32)
    if capacity is None:
        check(L.sf_eval_image_plan(_ptr(gt), width, B, W, H, _ptr(v), len(v), 0, dev, _ptr(count), None, None))
        capacity = int(count.max()) if B else 0
    capacity = int(capacity)
    iid, px = np.zeros((B, capacity), np.int32), np.zeros((B, capacity), np.uint32)
    check(L.sf_eval_image_plan(_ptr(gt), width, B, W, H, _ptr(v), len(v), capacity, dev, _ptr(count), _ptr(iid), _ptr(px)))
    return count, iid, px


def overlaps_images(gt, count, instance_id, masks, mask_image, valid_ids=INSTANCE_IDS, device=None):
    """sf_eval_overlaps_images(_device) -> table uint32 [P, capacity + 2] (torch: int32 on the device): per mask the covered pixels in each instance
    of its image, in void at [capacity], in all at [capacity + 1].  gt [B, H, W]; count [B] and instance_id [B, capacity]: image_plan's; masks
    [P, H * W] (or [P, H, W]) of bytes or bools, rows may be further apart than H * W; mask_image [P]: the image of each mask."""
    L = _lib()
    v = _valid(valid_ids)
    gt, width, tensors = _images(gt)
    B, H, W = (int(x) for x in gt.shape)
    n = H * W
    if tensors:
        import torch
        same = all(_is_tensor(t) and t.is_cuda and t.device == gt.device for t in (count, instance_id, masks, mask_image))
        if not same:
            raise ValueError("every array must be a tensor on the GPU of the images (or every one a numpy array)")
        if masks.dtype == torch.bool:
            masks = masks.view(torch.uint8)
        if masks.element_size() != 1:
            raise TypeError("masks of bytes")
        if masks.ndim == 3:
            masks = masks.reshape(masks.shape[0], -1)
        if masks.ndim != 2 or masks.shape[1] != n:
            raise ValueError("masks %s over images of %d pixels" % (tuple(masks.shape), n))
        P = int(masks.shape[0])
        if P > 1 and (masks.stride(1) != 1 or masks.stride(0) < n):
            masks = masks.contiguous()
        elif P == 1 and n > 1 and masks.stride(1) != 1:
            masks = masks.contiguous()
        stride = int(masks.stride(0)) if P > 1 else n
        for t in (count, instance_id, mask_image):
            if t.element_size() != 4 or t.dtype.is_floating_point:
                raise TypeError("counts, ids and mask_image of 32-bit integers")
        count, instance_id, mask_image = count.contiguous(), instance_id.contiguous(), mask_image.contiguous()
        capacity = int(instance_id.shape[1])
        if tuple(instance_id.shape) != (B, capacity) or count.numel() != B or mask_image.numel() != P:
            raise ValueError("a plan of %s / %s for %d images, %d image indices for %d masks" % (tuple(count.shape), tuple(instance_id.shape), B, mask_image.numel(), P))
        table = torch.zeros((P, capacity + 2), dtype=torch.int32, device=gt.device)
        check(L.sf_eval_overlaps_images_device(_ptr(gt), width, B, W, H, _ptr(v), len(v), capacity, _ptr(count), _ptr(instance_id), _ptr(masks), P, stride,
                                               _ptr(mask_image), _stream(gt), _ptr(table)))
        return table
    masks = np.asarray(masks)
    if masks.dtype == np.bool_:
        masks = masks.view(np.uint8)
    if masks.dtype.itemsize != 1:
        raise TypeError("masks of bytes")
    if masks.ndim == 3:
        masks = masks.reshape(masks.shape[0], -1)
    if masks.ndim != 2 or masks.shape[1] != n:
        raise ValueError("masks %s over images of %d pixels" % (masks.shape, n))
    P = masks.shape[0]
    if P > 1 and (masks.strides[1] != 1 or masks.strides[0] < n):
        masks = np.ascontiguousarray(masks)
    elif P == 1:
        masks = np.ascontiguousarray(masks)
    stride = int(masks.strides[0]) if P > 1 else n
    count = np.ascontiguousarray(count, np.uint32).reshape(-1)
    instance_id = np.ascontiguousarray(instance_id, np.int32)
    mask_image = np.ascontiguousarray(mask_image, np.uint32).reshape(-1)
    if instance_id.ndim != 2 or instance_id.shape[0] != B or len(count) != B or len(mask_image) != P:
        raise ValueError("a plan of %s / %s for %d images, %d image indices for %d masks" % (count.shape, instance_id.shape, B, len(mask_image), P))
    capacity = int(instance_id.shape[1])
    table = np.zeros((P, capacity + 2), np.uint32)
    check(L.sf_eval_overlaps_images(_ptr(gt), width, B, W, H, _ptr(v), len(v), capacity, _ptr(count), _ptr(instance_id), _ptr(masks), P, stride,
                                    _ptr(mask_image), -1 if device is None else int(device), _ptr(table)))
    return table


def ap2d_thresholds():
    """The ten overlap thresholds of the 2-D instance AP, bit for bit numpy's arange(0.5, 1., 0.05) (sf_eval_ap2d_thresholds)."""
    th = np.zeros(AP2D_OVERLAPS, np.float64)
    check(_lib().sf_eval_ap2d_thresholds(_ptr(th)))
    return th


class InstanceAP2D:
    """The AP over images (sf_eval_ap2d_*).  add(): a batch of images from their ids and masks; add_image(): one image from its plan and its rows of
    an overlap table; finish() -> {"ap": [n_valid, 10], "classes": {name: {"ap", "ap50%"}}, "all_ap", "all_ap_50%"}.  The result depends on neither
    the order of the images nor the order of an image's predictions."""

    def __init__(self, valid_ids=INSTANCE_IDS, names=INSTANCE_NAMES, min_region_size=100):
        self._L = _lib()
        self._h = C.c_void_p()
        self.valid_ids = _valid(valid_ids)
        self.names = tuple(names)
        if len(self.names) != len(self.valid_ids):
            raise ValueError("one name per valid class id")
        check(self._L.sf_eval_ap2d_create(_ptr(self.valid_ids), len(self.valid_ids), int(min_region_size), C.byref(self._h)))

    def close(self):
        if self._h.value:
            self._L.sf_eval_ap2d_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def add_image(self, instance_id, instance_pixels, pred_label, pred_conf, table):
        """instance_id, instance_pixels [G]; table [P, capacity + 2] with capacity >= G."""
        if _is_tensor(table):
            table = table.cpu().numpy()
        iid = np.ascontiguousarray(instance_id, np.int32).reshape(-1)
        px = np.ascontiguousarray(instance_pixels).astype(np.uint32, copy=False).reshape(-1)
        label = np.ascontiguousarray(pred_label, np.int32).reshape(-1)
        conf = np.ascontiguousarray(pred_conf, np.float64).reshape(-1)
        table = np.ascontiguousarray(table).view(np.uint32) if np.asarray(table).dtype.itemsize == 4 else np.ascontiguousarray(table, np.uint32)
        G, P = len(iid), len(label)
        if len(px) != G or len(conf) != P or table.ndim != 2 or table.shape[0] != P or table.shape[1] < G + 2:
            raise ValueError("a table of %s for %d predictions and %d instances" % (table.shape, P, G))
        check(self._L.sf_eval_ap2d_add_image(self._h, G, _ptr(iid), _ptr(px), P, _ptr(label), _ptr(conf), _ptr(table), table.shape[1] - 2))

    def add(self, gt, masks, mask_image, pred_label, pred_conf, device=None, capacity=None):
        """gt [B, H, W]; masks [P, H * W]; mask_image, pred_label, pred_conf [P].  numpy arrays (device: None = host), or tensors on a GPU with a
        capacity: the plan and the table are made there, and the counts and the table are read back once."""
        if _is_tensor(gt):
            import torch
            count, iid, px = image_plan(gt, self.valid_ids, capacity)
            mi = mask_image if _is_tensor(mask_image) else torch.from_numpy(np.ascontiguousarray(mask_image, np.int32)).to(gt.device)
            table = overlaps_images(gt, count, iid, masks, mi, self.valid_ids).cpu().numpy().view(np.uint32)
            count, iid, px = count.cpu().numpy().view(np.uint32), iid.cpu().numpy(), px.cpu().numpy().view(np.uint32)
            if len(count) and int(count.max()) > int(capacity):
                raise ValueError("an image holds %d instances, capacity %d" % (int(count.max()), int(capacity)))
            mask_image = mi.cpu().numpy()
        else:
            count, iid, px = image_plan(gt, self.valid_ids, capacity, device)
            table = overlaps_images(gt, count, iid, masks, mask_image, self.valid_ids, device)
        mask_image = np.asarray(mask_image).reshape(-1)
        label, conf = np.asarray(pred_label).reshape(-1), np.asarray(pred_conf, np.float64).reshape(-1)
        for b in range(len(count)):
            mine = np.flatnonzero(mask_image == b)
            G = int(count[b])
            self.add_image(iid[b, :G], px[b, :G], label[mine], conf[mine], table[mine])

    def finish(self):
        n = len(self.valid_ids)
        ap, cls, avg = np.zeros((n, AP2D_OVERLAPS), np.float64), np.zeros((n, 2), np.float64), np.zeros(2, np.float64)
        check(self._L.sf_eval_ap2d_finish(self._h, _ptr(ap), _ptr(cls), _ptr(avg)))
        classes = {name: {"ap": cls[i, 0], "ap50%": cls[i, 1]} for i, name in enumerate(self.names)}
        return {"ap": ap, "classes": classes, "all_ap": avg[0], "all_ap_50%": avg[1]}


def _dir_call(fn, pred_path, gt_path, output_file, device, *extra):
    L = _lib()
    text = C.c_void_p()
    out = None if not output_file else os.fsencode(str(output_file))
    check(getattr(L, fn)(os.fsencode(str(pred_path)), os.fsencode(str(gt_path)), out, *extra, -1 if device is None else int(device), C.byref(text)))
    try:
        return C.string_at(text).decode("utf-8", "replace") if text.value else ""
    finally:
        L.sf_free(text)


def evaluate_label_dir(pred_path, gt_path, output_file=None, device=None):
    """sf_eval_label_dir: evaluate_semantic_label.py on its files -> the text of its tables; the result file (default
    pred_path/semantic_label_evaluation.txt) is written.  device=None (the default) is the host path: DESIGN.md section 4o."""
    return _dir_call("sf_eval_label_dir", pred_path, gt_path, output_file, device)


def evaluate_instance_dir(pred_path, gt_path, output_file=None, min_region_size=100, device=None):
    """sf_eval_instance_dir: evaluate_semantic_instance.py on its files (default result file pred_path/semantic_instance_evaluation.txt)."""
    return _dir_call("sf_eval_instance_dir", pred_path, gt_path, output_file, device, int(min_region_size))


def evaluate_pixel_dir(pred_path, gt_path, output_file=None, device=None):
    """sf_eval_pixel_dir: evalPixelLevelSemanticLabeling.py on its PNG files (default result file pred_path/semantic_label.txt)."""
    return _dir_call("sf_eval_pixel_dir", pred_path, gt_path, output_file, device)


def evaluate_instance2d_dir(pred_path, gt_path, output_file=None, min_region_size=100, device=None):
    """sf_eval_instance2d_dir: evalInstanceLevelSemanticLabeling.py on its files -> the text of its table; the result file (default
    pred_path/semantic_instance.txt) is written.  device=None (the default) is the host path: DESIGN.md section 4p."""
    return _dir_call("sf_eval_instance2d_dir", pred_path, gt_path, output_file, device, int(min_region_size))


def export_ids(segs_json, aggregation_json, label_map_tsv):
    """sf_eval_export_ids -> (label_ids uint32 [V]: the nyu40id of every vertex, instance_ids uint32 [V]: objectId + 1; 0 = unannotated)."""
    L = _lib()
    args = (os.fsencode(str(segs_json)), os.fsencode(str(aggregation_json)), os.fsencode(str(label_map_tsv)))
    n = C.c_uint64(0)
    check(L.sf_eval_export_ids(*args, 0, None, None, C.byref(n)))
    label, inst = np.zeros(n.value, np.uint32), np.zeros(n.value, np.uint32)
    check(L.sf_eval_export_ids(*args, n.value, _ptr(label), _ptr(inst), C.byref(n)))
    return label, inst


def export_ground_truth(scan_path, label_map_file, type, output_file):
    """sf_eval_export_scan: export_train_mesh_for_evaluation.py on a scan folder.  type "label": a label id per line; "instance": the prediction
    format with its masks under pred_mask/ beside output_file; "instance-gt": label * 1000 + objectId + 1 per line, what evaluate_instance_dir
    reads as ground truth."""
    check(_lib().sf_eval_export_scan(os.fsencode(str(scan_path)), os.fsencode(str(label_map_file)), str(type).encode(), os.fsencode(str(output_file))))
