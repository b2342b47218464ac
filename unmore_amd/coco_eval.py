"""COCO box / mask AP and AR of a predictions file: the reference's last stage (COCO_evaluator/main.py -> COCOEvaluator -> COCOeval_opt,
i.e. pycocotools' cocoeval.py with Detectron2's compiled evaluateImg / accumulate) without pycocotools or Detectron2.

The two hot loops run on the device (csrc/coco_eval.hip): pairwise IoU -- of run-length masks straight from their strings, painted as
bit sets and intersected with AND + popcount, or of boxes in float64 in bbIou's operation order -- and the greedy per-threshold matching
of evaluateImg, one wave per (unit, area range, threshold).  An evaluation unit is one (image, category) pair.  What is left -- the
stable sort by score, cumulative sums, the precision envelope and the 101 recall points of `accumulate`, the twelve means of `summarize`
-- is numpy on the host over the small match tables.  There is no CPU fallback: off the GPU the device calls raise RuntimeError.

Data rules are pycocotools' (`loadRes`, `_prepare`): images = the ground truth's image ids, ascending (or `img_ids`); categories = the
ground truth's category ids, ascending; ignore = iscrowd; a ground truth's area is the file's `area`; a detection's area is its mask's
area for `segm` (its `bbox` is dropped, coco_evaluation.py:601-608) and w*h for `bbox`; a detection on an unknown image raises
ValueError.  Polygon ground truths (COCO's own annotation files) are rasterised on the device by pycocotools' rule (rle.from_polygons,
csrc/poly_rle.hip) when asked for: `COCOEvaluator(gt, polygons="rasterize")` converts them once at construction, `convert_polygons`
converts a file once; by default a polygon raises ValueError naming its annotation.  `bbox` reads only bbox / area / iscrowd and takes
any ground truth."""
import copy
import json
import os

import numpy as np

from . import rle

IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)      # cocoeval.py Params.setDetParams
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
AREA_RNG = np.array([[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]], dtype=np.float64)
AREA_LBL = ("all", "small", "medium", "large")
METRICS = ("AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AR100", "ARs", "ARm", "ARl")     # _derive_coco_results, :349-353


# ---------------------------------------------------------------------------------------------------------------- device calls
def _device(device, what):
    import torch
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"unmore_amd.coco_eval.{what} runs on the MI355X only (no CPU fallback)")
    return device


def _unit_tables(counts):
    """counts: list of (D, G) -> unit_start int32 [U+1], unit_nd int32 [U], unit_ng int32 [U], pair_offsets int64 [U+1]"""
    nd = np.array([d for d, _ in counts], dtype=np.int64)
    ng = np.array([g for _, g in counts], dtype=np.int64)
    start = np.concatenate([[0], np.cumsum(nd + ng)])
    pairs = np.concatenate([[0], np.cumsum(nd * ng)])
    if start[-1] >= 1 << 31 or (len(nd) and max(int(nd.max()), int(ng.max())) >= 1 << 31):
        raise ValueError("coco_eval: more than 2^31 records")
    return start.astype(np.int32), nd.astype(np.int32), ng.astype(np.int32), pairs.astype(np.int64)


def _dev(a, device):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _mask_records(units, what):
    """host-side checks before any launch: every unit's records as (H, W, bytes) and the unit's one size"""
    out = []
    for u, (dt, gt, crowd) in enumerate(units):
        if len(crowd) != len(gt):
            raise ValueError(f"{what}: unit {u}: {len(gt)} ground truths, {len(crowd)} iscrowd flags")
        recs = [rle._as_record(r, k, f"{what}: unit {u}") for k, r in enumerate(list(dt) + list(gt))]
        size = (recs[0][0], recs[0][1]) if recs else (1, 1)
        for k, (h, w, _) in enumerate(recs):
            if (h, w) != size:
                raise ValueError(f"{what}: unit {u}: record {k} has size {[h, w]}, the unit's first has {list(size)}: mixed mask sizes")
        out.append((recs, size, len(dt), len(gt)))
    return out


def _mask_iou_flat(units, device, what, prepared=None):
    """units: list of (dt_records, gt_records, iscrowd).  One umr_mask_iou call; returns the flat device tensors and the host tables:
    dict(inter int32 [P], iou f64 [P], area int32 [K], status numpy [K], start, nd, ng, pairs)"""
    import torch
    prepared = _mask_records(units, what) if prepared is None else prepared
    start, nd, ng, pairs = _unit_tables([(d, g) for _, _, d, g in prepared])
    U, K, P = len(prepared), int(start[-1]), int(pairs[-1])
    device = _device(device, what)
    from . import _lib as L
    from ._tables import workspace
    from .ops import _p, _stream
    with torch.cuda.device(device):
        inter = torch.zeros(P, dtype=torch.int32, device=device)
        iou = torch.zeros(P, dtype=torch.float64, device=device)
        area = torch.zeros(K, dtype=torch.int32, device=device)
        status = np.zeros(K, np.int32)
        if U and K:
            recs = [r for rs, _, _, _ in prepared for r in rs]
            nchars = np.array([len(c) for _, _, c in recs], dtype=np.int64)
            char_offsets = np.concatenate([[0], np.cumsum(nchars)]).astype(np.int64)
            nwords = np.array([(h * w + 63) // 64 for h, w, _ in recs], dtype=np.int64)
            word_offsets = np.concatenate([[0], np.cumsum(nwords)]).astype(np.int64)
            unit_size = np.array([[h, w, 0] for _, (h, w), _, _ in prepared], dtype=np.int64)
            crowd = np.zeros(K, np.uint8)
            for u, (_, _, c) in enumerate(units):
                crowd[start[u] + nd[u]:start[u + 1]] = [1 if x else 0 for x in c]
            total_chars, total_words = int(char_offsets[-1]), int(word_offsets[-1])
            chars = _dev(np.frombuffer(b"".join(c for _, _, c in recs) or b"\0", dtype=np.uint8).copy(), device)
            t_co, t_wo, t_us = _dev(char_offsets, device), _dev(word_offsets, device), _dev(unit_size, device)
            t_st, t_nd, t_po, t_cr = _dev(start, device), _dev(nd, device), _dev(pairs, device), _dev(crowd, device)
            st = torch.zeros(K, dtype=torch.int32, device=device)
            nbytes = L.lib().umr_mask_iou_workspace(K, total_chars, total_words)
            ws = workspace(nbytes, device)
            L.check(L.lib().umr_mask_iou(_p(chars), _p(t_co), K, total_chars, _p(t_us), _p(t_st), _p(t_nd), _p(t_po), _p(t_wo), _p(t_cr), U,
                                         max(h * w for _, (h, w), _, _ in prepared), int(nd.max()), int(ng.max()), P, total_words,
                                         _p(inter), _p(iou), _p(area), _p(st), _p(ws), nbytes, _stream()), "umr_mask_iou")
            status = st.cpu().numpy()                                            # the call's only synchronisation
    return {"inter": inter, "iou": iou, "area": area, "status": status, "start": start, "nd": nd, "ng": ng, "pairs": pairs}


def _split_units(flat, key_pairs=("inter", "iou")):
    out = []
    for u in range(len(flat["nd"])):
        D, G, r0, p0 = int(flat["nd"][u]), int(flat["ng"][u]), int(flat["start"][u]), int(flat["pairs"][u])
        rec = {k: flat[k][p0:p0 + D * G].view(D, G) for k in key_pairs if k in flat}
        if "area" in flat:
            rec["dt_area"], rec["gt_area"] = flat["area"][r0:r0 + D], flat["area"][r0 + D:r0 + D + G]
        out.append(rec)
    return out


def _raise_malformed(flat, what, payload):
    bad = np.flatnonzero(flat["status"])
    if bad.size:
        k = int(bad[0])
        why = "; ".join(t for b, t in rle._STATUS_BITS if int(flat["status"][k]) & b)
        err = ValueError(f"{what}: record {k} (detections then ground truths, unit after unit) is not a run-length string of its unit's "
                         f"mask size: {why}" + (f" (also malformed: records {', '.join(str(int(b)) for b in bad[1:])})" if bad.size > 1 else ""))
        err.status, err.units = flat["status"], payload      # what the well-formed records gave; a malformed one has area 0 and meets nothing
        raise err


def mask_iou_units(units, device="cuda"):
    """units: a list of (dt_records, gt_records, iscrowd), each one (image, category) pair whose masks share one size.  One device
    call for all of them; per unit a dict of device tensors: inter int32 [D,G] (intersection counts), iou float64 [D,G], dt_area int32
    [D], gt_area int32 [G].  A malformed string raises ValueError carrying `.status` (one word per record, the bits of
    umr_rle_decode) and `.units` (this list: the malformed record has area 0 and meets nothing, the others are unaffected)."""
    flat = _mask_iou_flat(units, device, "mask_iou")
    out = _split_units(flat)
    _raise_malformed(flat, "mask_iou", out)
    return out


def mask_iou(dt_records, gt_records, iscrowd, device="cuda"):
    """pycocotools.mask.iou for run-length records: float64 [D,G] on the device.  IoU = i / (a_d + a_g - i), i / a_d where
    iscrowd[g]; 0 when that denominator is 0.  Records as rle.decode takes them (strings, bytes or uncompressed count lists)."""
    return mask_iou_units([(dt_records, gt_records, iscrowd)], device)[0]["iou"]


def _box_iou_flat(units, device, what):
    import torch
    counts = []
    for u, (dt, gt, crowd) in enumerate(units):
        if len(crowd) != len(gt):
            raise ValueError(f"{what}: unit {u}: {len(gt)} ground truths, {len(crowd)} iscrowd flags")
        for k, b in enumerate(list(dt) + list(gt)):
            if len(b) != 4:
                raise ValueError(f"{what}: unit {u}: box {k} is not [x, y, w, h]")
        counts.append((len(dt), len(gt)))
    start, nd, ng, pairs = _unit_tables(counts)
    U, K, P = len(units), int(start[-1]), int(pairs[-1])
    device = _device(device, what)
    from . import _lib as L
    from .ops import _p, _stream
    with torch.cuda.device(device):
        iou = torch.zeros(P, dtype=torch.float64, device=device)
        if U and P:
            boxes = np.array([[float(v) for v in b] for dt, gt, _ in units for b in list(dt) + list(gt)], dtype=np.float64).reshape(K, 4)
            crowd = np.zeros(K, np.uint8)
            for u, (_, _, c) in enumerate(units):
                crowd[start[u] + nd[u]:start[u + 1]] = [1 if x else 0 for x in c]
            t_b, t_st, t_nd, t_po, t_cr = _dev(boxes, device), _dev(start, device), _dev(nd, device), _dev(pairs, device), _dev(crowd, device)
            L.check(L.lib().umr_box_iou(_p(t_b), _p(t_st), _p(t_nd), _p(t_po), _p(t_cr), U, K, int((nd.astype(np.int64) * ng).max()), P, _p(iou),
                                        _stream()), "umr_box_iou")
    return {"iou": iou, "start": start, "nd": nd, "ng": ng, "pairs": pairs}


def box_iou_units(units, device="cuda"):
    """units: a list of (dt_boxes, gt_boxes, iscrowd), boxes as [x, y, w, h]; per unit the float64 [D,G] IoU matrix on the device"""
    return [r["iou"] for r in _split_units(_box_iou_flat(units, device, "box_iou"), ("iou",))]


def box_iou(dt_boxes, gt_boxes, iscrowd, device="cuda"):
    """pycocotools.mask.iou for [x, y, w, h] boxes (maskApi.c bbIou, operation by operation in float64): float64 [D,G] on the device"""
    return box_iou_units([(dt_boxes, gt_boxes, iscrowd)], device)[0]


def _match_flat(iou, nd, ng, pairs, dt_area, gt_area, gt_crowd, area_rng, thrs, max_det, device):
    """one umr_coco_match call over flat tables; dt_area / gt_area float64 and gt_crowd uint8 device tensors in unit order.  Returns
    numpy: dtm, dtg, dtig [sum D * A * T], gtig [sum G * A], gtm [sum G * A * T] and the offsets det_off, gt_off"""
    import torch
    from . import _lib as L
    from .ops import _p, _stream
    area_rng = np.ascontiguousarray(area_rng, dtype=np.float64).reshape(-1, 2)
    thrs = np.ascontiguousarray(thrs, dtype=np.float64).reshape(-1)
    A, T, U = len(area_rng), len(thrs), len(nd)
    det_off = np.concatenate([[0], np.cumsum(nd.astype(np.int64))]).astype(np.int64)
    gt_off = np.concatenate([[0], np.cumsum(ng.astype(np.int64))]).astype(np.int64)
    ND, NG = int(det_off[-1]), int(gt_off[-1])
    with torch.cuda.device(device):
        dtm = torch.zeros(ND * A * T, dtype=torch.uint8, device=device)
        dtg = torch.full((ND * A * T,), -1, dtype=torch.int32, device=device)
        dtig = torch.zeros(ND * A * T, dtype=torch.uint8, device=device)
        gtig = torch.zeros(NG * A, dtype=torch.uint8, device=device)
        gtm = torch.zeros(NG * A * T, dtype=torch.uint8, device=device)
        if U:
            t_po, t_nd, t_ng, t_do, t_go = _dev(pairs, device), _dev(nd, device), _dev(ng, device), _dev(det_off, device), _dev(gt_off, device)
            t_ar, t_th = _dev(area_rng, device), _dev(thrs, device)
            assert dt_area.dtype == torch.float64 and gt_area.dtype == torch.float64 and gt_crowd.dtype == torch.uint8 and iou.dtype == torch.float64
            assert dt_area.numel() == ND and gt_area.numel() == NG and gt_crowd.numel() == NG and iou.numel() == int(pairs[-1])
            L.check(L.lib().umr_coco_match(_p(iou), _p(t_po), int(pairs[-1]), _p(t_nd), _p(t_ng), _p(t_do), ND, _p(t_go), NG, _p(dt_area.contiguous()),
                                           _p(gt_area.contiguous()), _p(gt_crowd.contiguous()), _p(t_ar), A, _p(t_th), T, int(max_det), U,
                                           _p(dtm), _p(dtg), _p(dtig), _p(gtig), _p(gtm), _stream()), "umr_coco_match")
        return {"dtm": dtm.cpu().numpy(), "dtg": dtg.cpu().numpy(), "dtig": dtig.cpu().numpy(), "gtig": gtig.cpu().numpy(),
                "gtm": gtm.cpu().numpy(), "det_off": det_off, "gt_off": gt_off, "A": A, "T": T}


def _split_match(m, nd, ng):
    A, T, out = m["A"], m["T"], []
    for u in range(len(nd)):
        D, G, d0, g0 = int(nd[u]), int(ng[u]), int(m["det_off"][u]), int(m["gt_off"][u])
        out.append({"dtm": m["dtm"][d0 * A * T:(d0 + D) * A * T].reshape(A, T, D).astype(bool),
                    "dtg": m["dtg"][d0 * A * T:(d0 + D) * A * T].reshape(A, T, D),
                    "dtig": m["dtig"][d0 * A * T:(d0 + D) * A * T].reshape(A, T, D).astype(bool),
                    "gtig": m["gtig"][g0 * A:(g0 + G) * A].reshape(A, G).astype(bool),
                    "gtm": m["gtm"][g0 * A * T:(g0 + G) * A * T].reshape(A, T, G).astype(bool)})
    return out


def match_units(units, area_rng=AREA_RNG, thrs=IOU_THRS, max_det=100, device="cuda"):
    """pycocotools' evaluateImg for every (unit, area range, threshold) in one device call.  units: a list of (iou, dt_area, gt_area,
    gt_iscrowd): iou a float64 [D,G] device tensor whose rows are the detections in descending-score order, the areas and flags
    array-likes.  Per unit a dict of numpy arrays: dtm bool [A,T,D] (matched), dtg int32 [A,T,D] (the ground truth's index or -1), dtig
    bool [A,T,D] (ignored), gtig bool [A,G], gtm bool [A,T,G].  Detections beyond max_det come back as (False, -1, True)."""
    import torch
    device = _device(device, "match_units")
    counts = []
    for u, (iou, da, ga, gc) in enumerate(units):
        D, G = len(da), len(ga)
        if tuple(iou.shape) != (D, G) or len(gc) != G:
            raise ValueError(f"match_units: unit {u}: iou {tuple(iou.shape)} against {D} detections, {G} ground truths, {len(gc)} iscrowd flags")
        counts.append((D, G))
    _, nd, ng, pairs = _unit_tables(counts)
    cat = lambda xs, dt: np.concatenate([np.asarray(x, dtype=dt).reshape(-1) for x in xs] + [np.zeros(0, dt)])
    with torch.cuda.device(device):
        iou = torch.cat([i.to(device=device, dtype=torch.float64).reshape(-1) for i, _, _, _ in units] +
                        [torch.zeros(0, dtype=torch.float64, device=device)])
        m = _match_flat(iou, nd, ng, pairs, _dev(cat([x[1] for x in units], np.float64), device), _dev(cat([x[2] for x in units], np.float64), device),
                        _dev(cat([[1 if c else 0 for c in x[3]] for x in units], np.uint8), device), area_rng, thrs, max_det, device)
    return _split_match(m, nd, ng)


# ---------------------------------------------------------------------------------------------------------------- accumulate / summarize
def accumulate(per_unit, scores, unit_cat, n_cats, max_dets, rec_thrs=REC_THRS):
    """pycocotools' accumulate over the match tables.  per_unit: the dicts of `match_units` in (category, image) order, None for a
    unit without detections and ground truths; scores: per unit the detections' scores in their (descending) order; unit_cat: per unit
    its category index.  Returns precision [T,R,K,A,M], recall [T,K,A,M], scores [T,R,K,A,M], -1 where undefined."""
    first = next((e for e in per_unit if e is not None), None)
    A, T = (first["dtm"].shape[0], first["dtm"].shape[1]) if first is not None else (len(AREA_RNG), len(IOU_THRS))
    R, K, M = len(rec_thrs), n_cats, len(max_dets)
    precision, recall, sc = -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M)), -np.ones((T, R, K, A, M))
    for k in range(K):
        E = [(e, np.asarray(s, np.float64)) for e, s, c in zip(per_unit, scores, unit_cat) if c == k and e is not None]
        if not E:
            continue
        for a in range(A):
            gt_ig = np.concatenate([e["gtig"][a] for e, _ in E])
            npig = np.count_nonzero(gt_ig == 0)
            if npig == 0:
                continue
            for m, max_det in enumerate(max_dets):
                dt_scores = np.concatenate([s[0:max_det] for _, s in E])
                inds = np.argsort(-dt_scores, kind="mergesort")
                sorted_scores = dt_scores[inds]
                dtm = np.concatenate([e["dtm"][a][:, 0:max_det] for e, _ in E], axis=1)[:, inds]
                dt_ig = np.concatenate([e["dtig"][a][:, 0:max_det] for e, _ in E], axis=1)[:, inds]
                tp_sum = np.cumsum(np.logical_and(dtm, np.logical_not(dt_ig)), axis=1).astype(dtype=float)
                fp_sum = np.cumsum(np.logical_and(np.logical_not(dtm), np.logical_not(dt_ig)), axis=1).astype(dtype=float)
                nd = len(dt_scores)
                for t in range(T):
                    tp, fp = tp_sum[t], fp_sum[t]
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    pr = np.maximum.accumulate(pr[::-1])[::-1]                   # the right-to-left running maximum
                    idx = np.searchsorted(rc, rec_thrs, side="left")
                    ok = idx < nd                                                # zeros beyond the last reachable recall
                    q, ss = np.zeros(R), np.zeros(R)
                    q[ok], ss[ok] = pr[idx[ok]], sorted_scores[idx[ok]]
                    precision[t, :, k, a, m], sc[t, :, k, a, m] = q, ss
    return {"precision": precision, "recall": recall, "scores": sc}


def summarize(ev, max_dets, iou_thrs=IOU_THRS):
    """the twelve statistics of COCOevalMaxDets.summarize (the AP rows use max_dets[2]); -1 where no entry is defined"""
    def one(ap, iou_thr=None, area="all", max_det=100):
        aind = [i for i, lbl in enumerate(AREA_LBL) if lbl == area]
        mind = [i for i, md in enumerate(max_dets) if md == max_det]
        s = ev["precision"] if ap == 1 else ev["recall"]
        if iou_thr is not None:
            s = s[np.where(iou_thr == iou_thrs)[0]]
        s = s[:, :, :, aind, mind] if ap == 1 else s[:, :, aind, mind]
        return -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])
    md = max_dets
    return np.array([one(1, max_det=md[2]), one(1, iou_thr=.5, max_det=md[2]), one(1, iou_thr=.75, max_det=md[2]),
                     one(1, area="small", max_det=md[2]), one(1, area="medium", max_det=md[2]), one(1, area="large", max_det=md[2]),
                     one(0, max_det=md[0]), one(0, max_det=md[1]), one(0, max_det=md[2]),
                     one(0, area="small", max_det=md[2]), one(0, area="medium", max_det=md[2]), one(0, area="large", max_det=md[2])], dtype=np.float64)


# ---------------------------------------------------------------------------------------------------------------- polygon ground truths
def _is_polygon(seg):
    return isinstance(seg, (list, tuple))


def convert_polygons(gt_or_path, out_path=None, device="cuda"):
    """the one-time conversion of a ground-truth file whose annotations carry polygon segmentations (COCO's instances_*.json and the
    class-agnostic files made from it): every polygon `segmentation` becomes the run-length record pycocotools' annToRLE gives, in one
    `rle.from_polygons` call with the sizes of the ground truth's `images`.  Run-length segmentations, `area`, `bbox` and everything else
    stay as the file has them.  Returns the converted ground truth (the input is not modified) and writes it to out_path when given."""
    gt = gt_or_path
    if not isinstance(gt, dict):
        with open(gt) as f:
            gt = json.load(f)
    size_of = {im["id"]: (int(im["height"]), int(im["width"])) for im in gt["images"]}
    which = [i for i, g in enumerate(gt["annotations"]) if _is_polygon(g.get("segmentation"))]
    for i in which:
        g = gt["annotations"][i]
        if g["image_id"] not in size_of:
            raise ValueError(f"convert_polygons: annotation {g.get('id')!r} is on image {g['image_id']!r}, which the ground truth does not have")
    out = dict(gt)
    if which:
        anns = gt["annotations"]
        recs = rle.from_polygons([anns[i]["segmentation"] for i in which], [size_of[anns[i]["image_id"]] for i in which], device=device)
        out["annotations"] = list(anns)
        for i, rec in zip(which, recs):
            out["annotations"][i] = dict(anns[i], segmentation=rec)
    if out_path is not None:
        with open(out_path, "w") as f:
            json.dump(out, f)
    return out


# ---------------------------------------------------------------------------------------------------------------- the evaluator
class COCOEvaluator:
    """The surface COCO_evaluator/coco_evaluation.py:37-220 gives main.py: reset(), process(image_id, coco_instances), evaluate(img_ids).
    gt: the path of a COCO ground-truth file or the loaded dict.  evaluate() returns {"bbox": {...}, "segm": {...}} with the twelve names
    of METRICS, values x100 and nan where the statistic is -1; afterwards `.eval[task]` holds precision [T,R,K,A,M], recall [T,K,A,M] and
    scores [T,R,K,A,M] (float64, -1 where undefined) and `.stats[task]` the twelve raw statistics.  polygons: "raise" (a polygon
    ground truth makes the segm task raise ValueError) or "rasterize" (every polygon ground truth is converted here, once, by
    `convert_polygons`; the segm task then sees run-length records only)."""

    def __init__(self, gt, tasks=("bbox", "segm"), max_dets_per_image=None, device="cuda", polygons="raise"):
        if polygons not in ("raise", "rasterize"):
            raise ValueError(f"COCOEvaluator: polygons={polygons!r}; 'raise' or 'rasterize' expected")
        if not isinstance(gt, dict):
            with open(gt) as f:
                gt = json.load(f)
        self.gt = convert_polygons(gt, device=device) if polygons == "rasterize" else gt
        self.tasks = tuple(tasks)
        for t in self.tasks:
            if t not in ("bbox", "segm"):
                raise ValueError(f"COCOEvaluator: unknown task {t!r} (bbox and segm are evaluated)")
        self.max_dets = [1, 10, 100 if max_dets_per_image is None else int(max_dets_per_image)]     # coco_evaluation.py:115-119
        self.device = device
        self.eval, self.stats = {}, {}
        self.reset()

    def reset(self):
        self._predictions = []

    def process(self, image_id, coco_instances):
        self._predictions.append({"image_id": image_id, "instances": coco_instances})

    def evaluate(self, img_ids=None):
        if len(self._predictions) == 0:
            return {}
        results = [r for p in self._predictions for r in p["instances"]]
        out = {}
        if len(results) == 0:                                                    # "cocoapi does not handle empty results very well"
            return {task: {m: float("nan") for m in METRICS} for task in sorted(self.tasks)}
        plans = {task: self._plan(task, results, img_ids) for task in sorted(self.tasks)}      # every argument error before any launch
        for task in sorted(self.tasks):
            self.eval[task], self.stats[task] = self._evaluate_task(task, *plans[task])
            out[task] = {m: float(s * 100 if s >= 0 else "nan") for m, s in zip(METRICS, self.stats[task])}
        return copy.deepcopy(out)

    # the host side of one task: pycocotools' loadRes / _prepare rules, the units in (category, image) order, the argument checks
    def _plan(self, task, results, img_ids):
        gt = self.gt
        known = set(im["id"] for im in gt["images"])
        for r in results:
            if r["image_id"] not in known:
                raise ValueError(f"COCOEvaluator: a detection is on image {r['image_id']!r}, which the ground truth does not have")
        imgs = sorted(known) if img_ids is None else sorted(set(img_ids))
        cats = sorted(set(c["id"] for c in gt["categories"]))
        max_dets = sorted(self.max_dets)
        gts, dts = {}, {}
        for g in gt["annotations"]:
            if task == "segm" and _is_polygon(g.get("segmentation")):
                raise ValueError(f"COCOEvaluator: ground-truth annotation {g.get('id')!r} has a polygon segmentation; the segm task takes "
                                 "run-length segmentations (pass polygons='rasterize', or convert the file once with convert_polygons)")
            gts.setdefault((g["image_id"], g["category_id"]), []).append(g)
        for r in results:
            dts.setdefault((r["image_id"], r["category_id"]), []).append(r)
        key = "segmentation" if task == "segm" else "bbox"
        units, scores, unit_cat, gt_area, gt_crowd = [], [], [], [], []
        for k, cat in enumerate(cats):
            for img in imgs:
                g, d = gts.get((img, cat), []), dts.get((img, cat), [])
                order = np.argsort([-float(x["score"]) for x in d], kind="mergesort")[:max_dets[-1]]      # stable, as computeIoU
                d = [d[i] for i in order]
                crowd = [int(x.get("iscrowd", 0)) for x in g]
                units.append(([x[key] for x in d], [x[key] for x in g], crowd))
                scores.append(np.array([float(x["score"]) for x in d], dtype=np.float64))
                unit_cat.append(k)
                gt_area += [float(x["area"]) for x in g]
                gt_crowd += crowd
        prepared = _mask_records(units, "COCOEvaluator") if task == "segm" else None
        return units, prepared, scores, unit_cat, len(cats), gt_area, gt_crowd, max_dets

    # one task: IoU -> matches (device) -> accumulate -> summarize (host)
    def _evaluate_task(self, task, units, prepared, scores, unit_cat, n_cats, gt_area, gt_crowd, max_dets):
        import torch
        flat = (_mask_iou_flat(units, self.device, "COCOEvaluator", prepared) if task == "segm" else
                _box_iou_flat(units, self.device, "COCOEvaluator"))
        device = flat["iou"].device
        nd, ng, start = flat["nd"], flat["ng"], flat["start"]
        if task == "segm":
            _raise_malformed(flat, "COCOEvaluator", None)
            det_idx = np.concatenate([np.arange(start[u], start[u] + nd[u]) for u in range(len(nd))] + [np.zeros(0, np.int64)]).astype(np.int64)
            dt_area = flat["area"][_dev(det_idx, device)].to(torch.float64)      # a detection's area is its mask's
        else:
            dt_area = _dev(np.array([float(b[2]) * float(b[3]) for dt, _, _ in units for b in dt], dtype=np.float64), device)
        m = _match_flat(flat["iou"], nd, ng, flat["pairs"], dt_area, _dev(np.array(gt_area, dtype=np.float64), device),
                        _dev(np.array(gt_crowd, dtype=np.uint8), device), AREA_RNG, IOU_THRS, max_dets[-1], device)
        per_unit = [e if nd[u] + ng[u] > 0 else None for u, e in enumerate(_split_match(m, nd, ng))]
        ev = accumulate(per_unit, scores, unit_cat, n_cats, max_dets)
        return ev, summarize(ev, max_dets)


def evaluate_ap(gt_annotation_path, pred_annotation_path, evaluator, result_folder):
    """COCO_evaluator/main.py:24-70: the predictions file (a list of records) grouped by image, `score` defaulting to `weight` or 1 and
    `id` to the record's position, through `evaluator`; writes <result_folder>/ap_score.json and returns its contents"""
    with open(pred_annotation_path) as f:
        preds = json.load(f)
    by_image = {}
    for i, ann in enumerate(preds):
        if ann is None:
            continue
        ann.setdefault("id", i)
        by_image.setdefault(ann["image_id"], []).append(ann)
    evaluator.reset()
    for image_id, anns in by_image.items():
        for ann in anns:
            if "score" not in ann:
                ann["score"] = ann["weight"] if "weight" in ann else 1
        evaluator.process(image_id=image_id, coco_instances=anns)
    results = evaluator.evaluate()
    results["pred_annotation_path"] = pred_annotation_path
    results["gt_annotation_path"] = gt_annotation_path
    results["number_of_images"] = len(by_image)
    results["number_of_annotations"] = len(preds)
    os.makedirs(result_folder, exist_ok=True)
    with open(os.path.join(result_folder, "ap_score.json"), "w") as f:
        json.dump(results, f, indent=2)
    return results
