"""Cases of the 2-D instance task for tests/test_instance2d.py and tests/test_instance2d_gpu.py: seeded id images with their
masks, built in memory; the brute-force checker tests/instance2d_checker.c behind ctypes; the AP restated from the section in plain numpy, from the
images and the masks themselves (no plan, no table); and the hand-made file case that tests/golden/make_instance2d_golden.py runs the reference's
script on."""
import atexit
import ctypes as C
import hashlib
import os
import shutil
import subprocess
import tempfile

import numpy as np

from scannet_amd import evaluation as ev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKER = os.path.join(ROOT, "tests", "instance2d_checker.c")
INSTANCE_IDS = np.array(ev.INSTANCE_IDS, np.int32)
_checker = []


def build_checker():
    """gcc -O2; None when there is no gcc."""
    if _checker:
        return _checker[0]
    if shutil.which("gcc") is None:
        _checker.append(None)
        return None
    d = tempfile.mkdtemp(prefix="i2_checker_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    so = os.path.join(d, "libinstance2d_checker.so")
    subprocess.run(["gcc", "-O2", "-shared", "-fPIC", "-o", so, CHECKER], check=True)
    L = C.CDLL(so)
    vp, i64 = C.c_void_p, C.c_int64
    L.i2c_plan.argtypes = [vp, i64, vp, C.c_int, vp, vp]
    L.i2c_plan.restype = i64
    L.i2c_overlaps.argtypes = [vp, i64, vp, C.c_int, vp, i64, vp, vp]
    L.i2c_overlaps.restype = None
    _checker.append(L)
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes())
    return h.hexdigest()


def as_values(a):
    """What the library reads in a pixel: the bits as an unsigned integer, in int64."""
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize]).astype(np.int64)


def check_plan(L, gt, valid=INSTANCE_IDS):
    """gt [B, H, W] -> per image (ids int64 [G] ascending, pixels int64 [G])"""
    plans = []
    for img in as_values(gt):
        flat = np.ascontiguousarray(img.reshape(-1))
        ids, px = np.zeros(len(flat), np.int64), np.zeros(len(flat), np.int64)
        G = L.i2c_plan(_p(flat), len(flat), _p(valid), len(valid), _p(ids), _p(px))
        plans.append((ids[:G].copy(), px[:G].copy()))
    return plans


def check_table(L, gt, plans, masks, mask_image, capacity, valid=INSTANCE_IDS):
    """-> table int64 [P, capacity + 2], the layout of sf_eval_overlaps_images"""
    vals = as_values(gt)
    masks = np.ascontiguousarray(masks).view(np.uint8).reshape(len(mask_image), -1)
    table = np.zeros((len(mask_image), capacity + 2), np.int64)
    for p, b in enumerate(mask_image):
        flat = np.ascontiguousarray(vals[b].reshape(-1))
        ids = plans[b][0]
        row = np.zeros(len(ids) + 2, np.int64)
        m = np.ascontiguousarray(masks[p])
        L.i2c_overlaps(_p(flat), len(flat), _p(valid), len(valid), _p(ids), len(ids), _p(m), _p(row))
        table[p, :len(ids)] = row[:len(ids)]
        table[p, capacity:] = row[len(ids):]
    return table


def plan_arrays(plans, capacity=None):
    """The checker's plans in the layout of sf_eval_image_plan: (count [B], ids [B, capacity], pixels [B, capacity]), zeros beyond an image's count."""
    count = np.array([len(p[0]) for p in plans], np.uint32)
    capacity = int(count.max()) if capacity is None and len(count) else int(capacity or 0)
    ids, px = np.zeros((len(plans), capacity), np.int32), np.zeros((len(plans), capacity), np.uint32)
    for b, (i, c) in enumerate(plans):
        ids[b, :len(i)], px[b, :len(i)] = i, c
    return count, ids, px


# ---- seeded images ----

CLASSES = (3, 4, 5, 7, 39)
OTHER_VALUES = (0, 0, 1, 2, 13, 40, 255, 999, 1000, 2999, 13001, 40000, 65535)   # neither an instance nor void, whatever the width leaves of them
VOID_VALUES = (3, 5, 39, 39)


def image_batch(seed, batch, width, height, dtype=np.uint16, n_inst=12, masks_per_image=4, top=None):
    """-> (gt [B, H, W] of dtype, masks uint8 [P, H * W], mask_image uint32 [P], labels int32 [P], confs float64 [P]).  Images of rectangles: instances
    (some below 100 pixels), void (raw values that are class ids), values that are neither, the type's largest value and, for 4 bytes, values above
    2^31 and 2^32 - 1.  Masks: rectangles around instances (exact, shifted, half), over void, empty ones; values 1, 2 and 255; labels of valid and
    of no class; confidences with ties."""
    rng = np.random.default_rng(seed)
    info = np.iinfo(dtype)
    gt = np.zeros((batch, height, width), np.int64)
    masks, mask_image, labels, confs = [], [], [], []
    grid = np.array([0.1, 0.25, 0.5, 0.5, 0.75, 0.9, 0.9, 0.99])

    def rect():
        x0, y0 = int(rng.integers(0, width)), int(rng.integers(0, height))
        return x0, y0, min(width, x0 + int(rng.integers(1, max(2, width // 2)))), min(height, y0 + int(rng.integers(1, max(2, height // 2))))
    for b in range(batch):
        boxes = []
        for v in rng.choice(OTHER_VALUES, size=3):
            x0, y0, x1, y1 = rect()
            gt[b, y0:y1, x0:x1] = min(int(v), info.max)
        for v in rng.choice(VOID_VALUES, size=2):
            x0, y0, x1, y1 = rect()
            gt[b, y0:y1, x0:x1] = v
        for k in range(n_inst if info.max >= 3000 else 0):
            x0, y0, x1, y1 = rect()
            label = int(rng.choice(CLASSES))
            value = label * 1000 + k + 1
            if value <= info.max:
                gt[b, y0:y1, x0:x1] = value
                boxes.append((x0, y0, x1, y1, label))
        if info.max > 65535:
            x0, y0, x1, y1 = rect()
            gt[b, y0:y1, x0:x1] = int(rng.choice([2 ** 31 + 5001, 2 ** 32 - 1, 5001 + 2 ** 20]))
        for _ in range(masks_per_image):
            x0, y0, x1, y1, label = boxes[int(rng.integers(0, len(boxes)))] if boxes else rect() + (5,)
            kind = rng.choice(["exact", "exact", "shift", "half", "void", "empty", "wrong", "invalid"])
            if kind == "shift":
                s = int(rng.integers(-3, 4))
                x0, x1 = max(0, x0 + s), min(width, x1 + s)
            elif kind == "half":
                y1 = y0 + max(1, (y1 - y0) // 2)
            elif kind == "void":
                x0, y0, x1, y1 = rect()
            elif kind == "wrong":
                label = int(rng.choice([c for c in CLASSES if c != label]))
            elif kind == "invalid":
                label = int(rng.choice([0, 1, 2, 13, 40, -1, 5000]))
            m = np.zeros((height, width), np.uint8)
            if kind != "empty":
                m[y0:y1, x0:x1] = rng.choice([1, 2, 255])
            masks.append(m.reshape(-1))
            mask_image.append(b)
            labels.append(label)
            confs.append(rng.choice(grid) if rng.random() < 0.6 else rng.random())
    masks = np.stack(masks) if masks else np.zeros((0, width * height), np.uint8)
    return (np.ascontiguousarray(gt.astype(dtype)), masks, np.array(mask_image, np.uint32), np.array(labels, np.int32), np.array(confs, np.float64))


def distinct_ids_image(width, height, dtype=np.uint32, first=1):
    """Every pixel its own id, spread over the 18 classes: pixel i is class INSTANCE_IDS[i % 18], number first + i // 18 (below 1000)."""
    i = np.arange(width * height)
    return (INSTANCE_IDS[i % 18].astype(np.int64) * 1000 + first + i // 18).astype(dtype).reshape(1, height, width)


# ---- the AP restated from section 4p ----

class Image:
    """gt [H, W]; masks uint8 [P, H * W]; labels int32 [P]; confs float64 [P]"""

    def __init__(self, gt, masks, labels, confs):
        self.gt = np.ascontiguousarray(gt)
        self.labels = np.ascontiguousarray(labels, np.int32).reshape(-1)
        self.masks = np.ascontiguousarray(masks, np.uint8).reshape(len(self.labels), self.gt.size)
        self.confs = np.ascontiguousarray(confs, np.float64).reshape(-1)


def images_of(gt, masks, mask_image, labels, confs):
    return [Image(gt[b], masks[mask_image == b], labels[mask_image == b], confs[mask_image == b]) for b in range(len(gt))]


def ap_from_the_rule(images, valid=INSTANCE_IDS, min_region=100):
    """DESIGN.md section 4p 'Matching', from images and masks.  -> ap [n_valid, 10].  The two-score rule is applied as its closed form: of the
    predictions that exceed the threshold on an instance the highest score is the match and every other one a false positive."""
    th = np.arange(0.5, 1., 0.05)
    valid = [int(v) for v in valid]
    per_image = []
    for im in images:
        gt = as_values(im.gt).reshape(-1)
        cover = im.masks != 0
        size = cover.sum(1)
        void = np.isin(gt, valid)
        inst = [int(i) for i in np.unique(gt) if (i // 1000) in valid]
        member = np.stack([gt == i for i in inst]) if inst else np.zeros((0, len(gt)), bool)
        inter = cover.astype(np.int64) @ member.T.astype(np.int64) if len(inst) else np.zeros((len(size), 0), np.int64)
        per_image.append(dict(inst=inst, pixels=member.sum(1), inter=inter, size=size, void=(cover & void).sum(1), labels=im.labels, confs=im.confs))
    ap = np.full((len(valid), len(th)), np.nan)
    for ci, cls in enumerate(valid):
        for oi, t in enumerate(th):
            score, true, missed, has_gt, has_pred = [], [], 0, False, False
            for d in per_image:
                mine = [g for g, i in enumerate(d["inst"]) if i // 1000 == cls]
                preds = [p for p in range(len(d["labels"])) if d["labels"][p] == cls and d["size"][p] > 0]
                has_pred |= bool(preds)

                def overlap(g, p):
                    k = int(d["inter"][p, g])
                    return k / (int(d["pixels"][g]) + int(d["size"][p]) - k)
                for g in mine:
                    if d["pixels"][g] < min_region:
                        continue
                    has_gt = True
                    hits = sorted(d["confs"][p] for p in preds if d["inter"][p, g] > 0 and overlap(g, p) > t)
                    if not hits:
                        missed += 1
                        continue
                    score += hits
                    true += [0.0] * (len(hits) - 1) + [1.0]
                for p in preds:
                    if any(d["inter"][p, g] > 0 and overlap(g, p) > t for g in mine):
                        continue
                    ignore = int(d["void"][p]) + sum(int(d["inter"][p, g]) for g in mine if d["pixels"][g] < min_region)
                    if ignore / int(d["size"][p]) <= t:
                        score.append(d["confs"][p])
                        true.append(0.0)
            if not has_gt:
                continue
            if not has_pred:
                ap[ci, oi] = 0.0
                continue
            score, true = np.array(score, np.float64), np.array(true, np.float64)
            precision, recall = [], []
            for s in np.unique(score):
                at = score >= s
                tp, fn = true[at].sum(), true[~at].sum() + missed
                precision.append(tp / at.sum())
                recall.append(tp / (tp + fn))
            precision.append(1.0)
            recall.append(0.0)
            r = np.array([recall[0]] + recall + [0.0])
            ap[ci, oi] = np.dot(np.array(precision), np.convolve(r, [-0.5, 0, 0.5], "valid"))
    return ap


def averages_from_the_rule(ap):
    import warnings
    cls = np.stack([ap.mean(1), ap[:, 0]], 1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        avg = np.array([np.nanmean(ap), np.nanmean(ap[:, 0])])
    return cls, avg


# ---- the file case (bin/evaluate instance2d, evaluate_instance2d_dir; tests/golden/make_instance2d_golden.py runs the reference on the same) ----

def _rect(shape, x0, x1, y0, y1, value=1):
    m = np.zeros(shape, np.uint8)
    m[y0:y1, x0:x1] = value
    return m


def file_case():
    """-> [(list path relative to pred_path, gt uint16 [H, W], [(mask path relative to the list's folder, mask uint8 [H, W] or None: not written,
    label, confidence text)])].  What the images hold between them is listed in the issue of this feature and in DESIGN.md section 4p 'Golden'."""
    H, W = 96, 128
    a = np.zeros((H, W), np.uint16)
    a[10:50, 10:50] = 5001      # chair, 1600 pixels
    a[10:40, 60:100] = 5002     # chair, 1200
    a[60:90, 10:70] = 7001      # table, 1800
    a[50:58, 100:108] = 6001    # sofa, 64: below 100 pixels
    a[0:40, 110:128] = 3        # void: the raw value is a class id
    a[60:96, 110:128] = 1       # neither
    a[60:90, 75:100] = 4001     # bed, 750: ground truth and no prediction
    a[92:96, 0:8] = 65535
    preds_a = [
        ("masks/frame0_table.png", None, 7, "0.1"),                                             # listed twice: the later label and confidence hold
        ("masks/frame0_000.png", _rect((H, W), 14, 54, 10, 50, 1), 5, "0.9"),                  # chair 5001 shifted: overlap 1440 / 1760, matched up to 0.8
        ("masks/frame0_001.png", _rect((H, W), 10, 50, 12, 50, 255), 5, "0.8"),                # chair 5001 again: 1520 / 1600, the second match
        ("masks/frame0_002.png", _rect((H, W), 60, 100, 10, 40, 255), 5.0, "0.7"),             # chair 5002 exactly; the label as a float
        ("masks/frame0_table.png", _rect((H, W), 10, 70, 60, 80, 1), 7, "0.6"),                # table 7001: 1200 / 1800
        ("masks/frame0_004.png", _rect((H, W), 100, 108, 50, 58, 1), 6, "0.5"),                # on the small sofa: ignored
        ("masks/frame0_005.png", _rect((H, W), 108, 128, 0, 40, 255), 8, "0.55"),              # door: 720 of 800 pixels on void, ignored up to 0.85
        ("masks/frame0_006.png", np.zeros((H, W), np.uint8), 5, "0.99"),                       # empty: dropped
        ("masks/not_there.png", None, 13, "0.4"),                                              # no valid class: dropped, never opened
    ]
    b = np.zeros((H, W), np.uint16)
    b[20:60, 20:60] = 5001      # chair, 1600
    b[10:30, 70:120] = 9001     # window, 1000
    b[70:96, 0:16] = 16001      # curtain, 416: ground truth and no prediction
    b[70:96, 100:128] = 2
    preds_b = [
        ("masks/frame1_000.png", _rect((H, W), 40, 80, 20, 60, 1), 5, "0.85"),                 # chair: 800 / 2400, no match
        ("masks/frame1_001.png", _rect((H, W), 70, 120, 10, 30, 255), 9, "0.3"),               # window exactly
        ("masks/frame1_002.png", _rect((H, W), 100, 128, 70, 96, 1), 9, "0.95"),               # window over nothing: a false positive above the match
        ("masks/frame1_003.png", _rect((H, W), 70, 120, 12, 30, 1), 9, "0.3"),                 # window again, the same confidence: a tie
    ]
    h, w = 48, 64
    c = np.zeros((h, w), np.uint16)
    c[0:24, 0:32] = 5           # void
    c[24:48, 32:64] = 39        # void
    c[30:44, 4:28] = 34001      # sink, 336
    preds_c = [
        ("masks/frame2_000.png", _rect((h, w), 0, 32, 0, 24, 1), 34, "0.7"),                   # sink wholly on void: ignored at every threshold
        ("../masks/frame2_001.png", _rect((h, w), 40, 60, 4, 20, 255), 33, "1e-1"),            # toilet over nothing, no toilet anywhere; a path through ..
        ("masks/frame2_002.png", _rect((h, w), 4, 28, 30, 42, 1), 34, "0.65"),                 # sink: 288 / 336
    ]
    return [("frame0.txt", a, preds_a), ("frame1.txt", b, preds_b), ("sub/frame2.txt", c, preds_c)]


def write_file_case(root):
    """-> (pred_path, gt_path, sha256 of the arrays and the lists)."""
    from scannet_amd import filter2d
    pred_path, gt_path = os.path.join(root, "i2_pred"), os.path.join(root, "i2_gt")
    os.makedirs(gt_path)
    parts = []
    for rel, gt, preds in file_case():
        lst = os.path.join(pred_path, rel)
        os.makedirs(os.path.dirname(lst), exist_ok=True)
        filter2d.png_write_gray(os.path.join(gt_path, os.path.splitext(os.path.basename(rel))[0] + ".png"), gt)
        text = ""
        for mask_rel, mask, label, conf in preds:
            text += "%s %s %s\n" % (mask_rel, label, conf)
            if mask is not None:
                path = os.path.normpath(os.path.join(os.path.dirname(lst), mask_rel))
                os.makedirs(os.path.dirname(path), exist_ok=True)
                filter2d.png_write_gray(path, mask)
                parts.append(mask)
        open(lst, "w").write(text)
        parts += [gt, np.frombuffer(text.encode(), np.uint8)]
    return pred_path, gt_path, digest(*parts)


def file_case_images():
    """The file case as the rule sees it: the duplicate resolved, the dropped entries gone."""
    out = []
    for _, gt, preds in file_case():
        kept = {}
        for mask_rel, mask, label, conf in preds:
            kept[os.path.normpath(mask_rel)] = (mask if mask is not None else kept.get(os.path.normpath(mask_rel), (None,))[0], int(float(label)), float(conf))
        rows = [(m, l, c) for m, l, c in kept.values() if l in ev.INSTANCE_IDS]
        out.append(Image(gt, np.stack([m.reshape(-1) for m, _, _ in rows]), [l for _, l, _ in rows], [c for _, _, c in rows]))
    return out


def result_table(text):
    """The table of printResults in the script's stdout: from the first rule to the average."""
    lines = text.replace("\r", "\n").split("\n")
    a = lines.index("#" * 50)
    b = max(i for i, ln in enumerate(lines) if ln.startswith("average"))
    return lines[a:b + 1]
