"""Generate tests/golden/copy_paste.npz by running the REFERENCE's own CustomSimpleTrainer.copy_and_paste on the CPU.

Run where the reference tree is at hand, never on the GPU box:
    python tests/golden/make_golden_copy_paste.py /path/to/reference

What executes verbatim from the reference: cad/engine/train_loop.py, `CustomSimpleTrainer.__init__` and `.copy_and_paste` (:42-74,
:90-248), on pairs built as `run_step` builds them (:263): `copy_and_paste(copy.deepcopy(data[::-1]), data)`.  What cannot: Detectron2 is
absent, so placeholder `detectron2` modules answer the file's imports with minimal stand-ins written here -- `Instances` (fields,
`__getitem__`, `cat`, `.to`), `BitMasks` (`get_bounding_boxes` by Detectron2's published rule), `Boxes` (`scale`) and an empty
`SimpleTrainer`.  Every instance carries a `gt_source` field (0 = unlabeled / 1 = labeled, index), which the reference moves around
like any other field: that is where the fixture's `source` comes from.

The batch of nine items (pairs p = (8 - p, p)) reaches every branch: no copy (empty labeled item), empty unlabeled image, every copy
rejected by overlap, every copy rejected by an existing mask of area 0 (NaN), an existing instance erased to area 0 by three copies
that each cover less than half of it, different labeled and unlabeled sizes, the middle item paired with itself.  The reference's
draws depend on the seeds, sizes and instance counts only, so the generator first replays them (unmore_amd.copy_paste.draw_params on
equally seeded streams), looks for a seed whose draws allow the branches, shapes the masks of three items around those draws, and then
runs the reference on the global streams with that seed.  Only arrays are stored."""
import copy
import importlib.util
import os
import random
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from unmore_amd.copy_paste import draw_params  # noqa: E402
from copy_paste_common import blob_item, bounding_boxes  # noqa: E402

CFG = dict(rate=1.0, random_num=True, min_ratio=0.3, max_ratio=1.0)      # the stage-3 recipe's values
SIZES = [(48, 64), (40, 56), (33, 47), (41, 35), (48, 64), (37, 61), (30, 50), (44, 39), (45, 63)]
COUNTS = [4, 0, 3, 1, 4, 2, 3, 3, 2]


class Boxes:
    def __init__(self, tensor):
        self.tensor = tensor

    def scale(self, sx, sy):
        self.tensor[:, 0::2] *= sx
        self.tensor[:, 1::2] *= sy

    def __getitem__(self, item):
        return Boxes(self.tensor[item].view(-1, 4))

    def __len__(self):
        return self.tensor.shape[0]

    def to(self, device=None):
        return Boxes(self.tensor.to(device=device))

    @property
    def device(self):
        return self.tensor.device

    @staticmethod
    def cat(xs):
        return Boxes(torch.cat([x.tensor for x in xs], 0))


class BitMasks:
    def __init__(self, tensor):
        self.tensor = tensor.to(torch.bool)

    def __getitem__(self, item):
        m = self.tensor[item]
        return BitMasks(m.view(-1, *self.tensor.shape[1:]))

    def __len__(self):
        return self.tensor.shape[0]

    def to(self, device=None):
        return BitMasks(self.tensor.to(device=device))

    def get_bounding_boxes(self):
        return Boxes(bounding_boxes(self.tensor))

    @staticmethod
    def cat(xs):
        return BitMasks(torch.cat([x.tensor for x in xs], 0))


class Instances:
    def __init__(self, image_size, **fields):
        self._image_size = image_size
        self._fields = {}
        for k, v in fields.items():
            self._fields[k] = v

    def __setattr__(self, name, value):
        if name.startswith("_"):
            super().__setattr__(name, value)
        else:
            self._fields[name] = value

    def __getattr__(self, name):
        if name == "_fields" or name not in self._fields:
            raise AttributeError(name)
        return self._fields[name]

    def __len__(self):
        for v in self._fields.values():
            return len(v)
        raise NotImplementedError

    def __getitem__(self, item):
        return Instances(self._image_size, **{k: v[item] for k, v in self._fields.items()})

    def to(self, device=None):
        return Instances(self._image_size, **{k: v.to(device=device) for k, v in self._fields.items()})

    def get_fields(self):
        return self._fields

    @staticmethod
    def cat(xs):
        out = Instances(xs[0]._image_size)
        for k in xs[0]._fields:
            vs = [x._fields[k] for x in xs]
            out._fields[k] = torch.cat(vs, 0) if isinstance(vs[0], torch.Tensor) else type(vs[0]).cat(vs)
        return out


def load_reference(ref_root):
    d2, st, sti, eng = (types.ModuleType(n) for n in ("detectron2", "detectron2.structures", "detectron2.structures.instances",
                                                      "detectron2.engine"))
    sti.Instances, st.Instances, st.BitMasks, st.Boxes, st.instances = Instances, Instances, BitMasks, Boxes, sti
    eng.SimpleTrainer = type("SimpleTrainer", (), {"__init__": lambda self, *a, **k: None})
    d2.structures, d2.engine = st, eng
    for m in (d2, st, sti, eng):
        sys.modules[m.__name__] = m
    spec = importlib.util.spec_from_file_location("ref_train_loop", os.path.join(ref_root, "cad", "engine", "train_loop.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def pasted_masks(item, prm):
    """the chosen masks of `item` resized and pasted as the reference will: bool [n, h_new, w_new] in the frame's own coordinates"""
    choice, _, h_new, w_new, _, _ = prm
    m = item["masks"][torch.as_tensor(choice)]
    return F.interpolate(m[None].float(), size=(h_new, w_new), mode="bilinear", align_corners=False).bool()[0]


def build_items(seed):
    """the nine items for `seed`, or None when its draws do not allow the erase branch"""
    B = len(SIZES)
    prms = draw_params([COUNTS[B - 1 - p] for p in range(B)], SIZES, py_random=random.Random(seed), np_random=np.random.RandomState(seed), **CFG)
    if prms[8] is None or sorted(prms[8][0].tolist()) != [0, 1, 2] or prms[8][2] < 6 or prms[8][3] < 12:
        return None
    rng = np.random.RandomState(1000 + seed)
    items = [blob_item(rng, h, w, n) for (h, w), n in zip(SIZES, COUNTS)]
    # item 0 (labeled of pair 8): three adjacent vertical stripes and a blob
    H, W = SIZES[0]
    m = items[0]["masks"]
    for k in range(3):
        m[k] = False
        m[k, :, W // 2 - 9 + 6 * k:W // 2 - 3 + 6 * k] = True
    # item 2: its last mask is empty (pair 2's unlabeled item: area 0 -> NaN; pair 6's labeled item: an empty copy)
    items[2]["masks"][2] = False
    # item 5 (labeled of pair 3): both masks cover the whole frame
    items[5]["masks"][:] = True
    # item 3 (unlabeled of pair 3): one pixel inside the pasted frame: every copy covers it
    _, _, h_new, w_new, h_shift, w_shift = prms[3]
    items[3]["masks"][:] = False
    items[3]["masks"][0, h_shift + h_new // 2, w_shift + w_new // 2] = True
    # item 8 (unlabeled of pair 8): mask 0 = one row of the three pasted stripes' union, mask 1 = the whole frame
    _, _, h_new, w_new, h_shift, w_shift = prms[8]
    pm = pasted_masks(items[0], prms[8])
    row = h_new // 2
    run = pm[:, row].any(0)
    if any(2 * int((pm[k, row] & run).sum()) >= int(run.sum()) for k in range(3)):
        return None
    m = items[8]["masks"]
    m[:] = False
    m[0, h_shift + row, w_shift:w_shift + w_new] = run
    m[1] = True
    for it in items:
        it["boxes"] = bounding_boxes(it["masks"])
    return items, prms


def to_data(items, origin):
    data = []
    for it in items:
        n = it["masks"].shape[0]
        src = torch.stack([torch.full((n,), origin, dtype=torch.int64), torch.arange(n, dtype=torch.int64)], 1)
        inst = Instances(tuple(it["image"].shape[1:]), gt_boxes=Boxes(it["boxes"].clone()), gt_masks=BitMasks(it["masks"].clone()), gt_source=src)
        data.append({"image": it["image"].clone(), "instances": inst})
    return data


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = load_reference(sys.argv[1])
    trainer = ref.CustomSimpleTrainer(None, None, None, cfg=None, use_copy_paste=True, copy_paste_rate=CFG["rate"],
                                      copy_paste_random_num=CFG["random_num"], copy_paste_min_ratio=CFG["min_ratio"],
                                      copy_paste_max_ratio=CFG["max_ratio"])
    for seed in range(10000):
        built = build_items(seed)
        if built is None:
            continue
        items, prms = built
        B = len(items)
        data = to_data(items, 0)
        labeled = copy.deepcopy(to_data(items, 1)[::-1])                # run_step :263, with the labeled copies marked as such
        random.seed(seed)
        np.random.seed(seed)
        out = trainer.copy_and_paste(labeled, data)
        unchanged = [all(torch.equal(a, b) for a, b in ((o["image"], it["image"]), (o["instances"].gt_masks.tensor, it["masks"])))
                     and len(o["instances"]) == it["masks"].shape[0] for o, it in zip(out, items)]
        n_from_unl = [int((o["instances"].gt_source[:, 0] == 0).sum()) for o in out]
        # the branches, asserted on the reference's own outputs
        ok = (prms[7] is None and unchanged[7]                                               # no copy
              and not unchanged[1] and len(out[1]["instances"]) == len(prms[1][0])           # empty unlabeled image
              and unchanged[2] and unchanged[3]                                              # NaN reject; overlap reject
              and not unchanged[8] and n_from_unl[8] == 1                                    # an existing instance erased
              and not unchanged[4] and not unchanged[0])                                     # self-pairing and a mixed pair do copy
        if not ok:
            continue
        arrays = {"seed": np.int64(seed), "n_items": np.int64(B), "cfg": np.array([CFG["rate"], float(CFG["random_num"]), CFG["min_ratio"],
                                                                                  CFG["max_ratio"]])}
        for k, it in enumerate(items):
            arrays[f"in{k}_image"], arrays[f"in{k}_masks"], arrays[f"in{k}_boxes"] = it["image"].numpy(), it["masks"].numpy(), it["boxes"].numpy()
        for p in range(B):
            arrays[f"draw{p}_copy"] = np.int64(prms[p] is not None)
            if prms[p] is not None:
                choice, ratio, h_new, w_new, h_shift, w_shift = prms[p]
                arrays[f"draw{p}_choice"] = choice
                arrays[f"draw{p}_ratio"] = np.float64(ratio)
                arrays[f"draw{p}_geom"] = np.array([h_new, w_new, h_shift, w_shift], dtype=np.int64)
            inst = out[p]["instances"]
            arrays[f"out{p}_unchanged"] = np.int64(unchanged[p])
            arrays[f"out{p}_image"] = out[p]["image"].numpy()
            arrays[f"out{p}_masks"] = inst.gt_masks.tensor.numpy()
            arrays[f"out{p}_boxes"] = inst.gt_boxes.tensor.numpy()
            arrays[f"out{p}_source"] = inst.gt_source.numpy()
        path = os.path.join(HERE, "copy_paste.npz")
        np.savez_compressed(path, **arrays)
        print(f"seed {seed}: wrote {path} ({os.path.getsize(path)} bytes); instances out: {[len(o['instances']) for o in out]}, "
              f"unchanged: {unchanged}")
        return
    sys.exit("no seed reaches every branch")


if __name__ == "__main__":
    main()
