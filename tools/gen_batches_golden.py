"""Writes tests/golden/train_batches.npz: seeded random uint8 frames and what the REFERENCE's own dataset classes (data/REDS.py and
data/Vimeo.py, imported unmodified at run time) return from __getitem__ for them.  Build container only; TEST INFRASTRUCTURE.  Only data
is recorded: the seeds, the values of the dataset config, the frame bytes, the returned 'LRs' / 'HRs'.

The reference imports lmdb and cv2, which are not installed: empty stand-in modules are registered under those names before the import
(neither is called: the datasets get in-memory HR_env / LR_env objects whose begin().get(key) returns the frame bytes, so _init_lmdb never
runs).  torch.distributed.get_rank, which the constructors call without a process group, is patched to answer 0.  The key list the
constructors unpickle is written to a temporary directory.

A case = one dataset object, random.seed(seed), then __getitem__ for each of the case's indices in order (one process, as with n_workers: 0).
The frames are 24 x 40 HR / 6 x 10 LR random bytes (not related by a resize: the dataset never checks), 6 frames per clip, 2 clips; crop
16 / 4 at x4.  Seeds of the all-flags REDS cases are searched until all 8 flag combinations and both reverse outcomes occur; which flags a
sample drew is read off its output (the one combination of tests/batches_ref.py that reproduces it), and asserted to cover.

int(np.random.choice(list, 1)) of data/REDS.py:156 runs under the installed numpy 2.2 (a DeprecationWarning for the conversion of a
1-element array): the pre_seed cases come from the reference too.

    VMG_REFERENCE=<path of the reference checkout> python tools/gen_batches_golden.py
"""
import importlib.util
import itertools
import json
import os
import pickle
import random
import sys
import tempfile
import types
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import batches_ref as R  # noqa: E402

REF = os.environ.get("VMG_REFERENCE", "")
SCALE, HR_SHAPE, FRAMES, CLIPS = 4, (3, 24, 40), 6, 2
KEYS = {"REDS": ["000", "001"], "Vimeo": ["00001_0001", "00001_0002"]}
BASE = {"scale": SCALE, "num_frames": 3, "total_num_frames": FRAMES, "crop_size": 16, "image_shape": list(HR_SHAPE), "random_reverse": True,
        "use_hflip": True, "use_vflip": True, "use_rot": True, "use_mirrors": False, "pre_seed": None}
INDICES = [0, 1, 1]


class MemTxn:
    def __init__(self, table):
        self.table = table

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def get(self, key):
        return self.table[key]


class MemEnv:
    """What the datasets use of an lmdb environment: begin(write=False) as a context manager whose get(key) returns bytes."""

    def __init__(self, table):
        self.table = table

    def begin(self, write=False):
        return MemTxn(self.table)


def import_reference(name):
    if not os.path.isdir(REF):
        raise SystemExit("reference not present: the fixture can only be regenerated in the build container")
    for standin in ("lmdb", "cv2"):
        sys.modules.setdefault(standin, types.ModuleType(standin))
    spec = importlib.util.spec_from_file_location("vmg_ref_data_" + name, os.path.join(REF, "data", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def env_for(dataset, frames):
    """frames (CLIPS, FRAMES, H, W, 3) -> the key -> bytes table: REDS numbers a clip's frames from 0, Vimeo from 1."""
    first = 0 if dataset == "REDS" else 1
    return MemEnv({f"{key}_{first + f}".encode("ascii"): frames[c, f].tobytes() for c, key in enumerate(KEYS[dataset]) for f in range(FRAMES)})


def run_case(cls, dataset, cfg, seed, hr, lr, tmp):
    path = os.path.join(tmp, dataset + "_keys.pkl")
    with open(path, "wb") as f:
        pickle.dump({"keys": KEYS[dataset]}, f)
    ds = cls(dict(cfg, dataroot_HR="unused", dataroot_LR="unused", data_type="lmdb", cache_keys=path))   # seeds numpy with pre_seed + 0 + 1
    ds.HR_env, ds.LR_env = env_for(dataset, hr), env_for(dataset, lr)
    random.seed(seed)
    outs = []
    for i in INDICES:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", DeprecationWarning)
            item = ds[i]
        assert item["key"] == KEYS[dataset][i] and item["LRs"].dtype == torch.float32 and item["HRs"].dtype == torch.float32
        outs.append((item["LRs"].numpy(), item["HRs"].numpy()))
    return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])


def what_was_drawn(dataset, cfg, clip, hr, lr, LRs, HRs):
    """(start, reversed, y0, x0, hflip, vflip, rot) of one recorded sample: the one combination whose restatement has its bits."""
    T, c = cfg["num_frames"], cfg["crop_size"] // SCALE
    H, W = HR_SHAPE[1] // SCALE, HR_SHAPE[2] // SCALE
    starts = range(0, cfg["total_num_frames"] - T + 1) if dataset == "REDS" else [0]
    found = []
    for start, rev, y0, x0 in itertools.product(starts, (False, True), range(max(0, H - c) + 1), range(max(0, W - c) + 1)):
        fr = list(range(start, start + T))
        fr = fr[::-1] if rev else fr
        fr = fr + fr[::-1] if cfg["use_mirrors"] else fr
        for hf, vf, rot in itertools.product((False, True), repeat=3):
            if rot and min(c, H) != min(c, W):
                continue
            l, h = R.sample(hr[clip], lr[clip], fr, y0, x0, hf, vf, rot, c, SCALE)
            if l.shape == LRs.shape and np.array_equal(l.view(np.int32), LRs.view(np.int32)) and np.array_equal(h.view(np.int32), HRs.view(np.int32)):
                found.append((start, rev, y0, x0, hf, vf, rot))
    assert len(found) == 1, found
    return found[0]


def main():
    mods = {"REDS": import_reference("REDS").REDSDataset, "Vimeo": import_reference("Vimeo").VimeoDataset}
    torch.distributed.get_rank = lambda: 0   # the constructors ask without a process group
    rng = np.random.default_rng(20241101)
    hr = rng.integers(0, 256, (CLIPS, FRAMES, HR_SHAPE[1], HR_SHAPE[2], 3), dtype=np.uint8)
    lr = rng.integers(0, 256, (CLIPS, FRAMES, HR_SHAPE[1] // SCALE, HR_SHAPE[2] // SCALE, 3), dtype=np.uint8)
    data, cases = {"hr": hr, "lr": lr}, []

    def record(name, dataset, seed, **changes):
        cfg = dict(BASE, **changes)
        LRs, HRs = run_case(mods[dataset], dataset, cfg, seed, hr, lr, tmp)
        data[name + "/LRs"], data[name + "/HRs"] = LRs, HRs
        cases.append({"name": name, "dataset": dataset, "seed": seed, "indices": INDICES, "cfg": cfg})
        drawn = [what_was_drawn(dataset, cfg, INDICES[k], hr, lr, LRs[k], HRs[k]) for k in range(len(INDICES))] if not cfg["use_mirrors"] else []
        print(name, LRs.shape, HRs.shape, drawn)
        return drawn

    with tempfile.TemporaryDirectory() as tmp:
        # all flags on: seeds until the 8 combinations and both reverse outcomes have occurred
        combos, reverses, seed = set(), set(), 0
        while len(combos) < 8 or len(reverses) < 2:
            before = (len(combos), len(reverses))
            cfg = dict(BASE)
            LRs, HRs = run_case(mods["REDS"], "REDS", cfg, seed, hr, lr, tmp)
            drawn = [what_was_drawn("REDS", cfg, INDICES[k], hr, lr, LRs[k], HRs[k]) for k in range(len(INDICES))]
            new_c, new_r = {d[4:] for d in drawn} - combos, {d[1] for d in drawn} - reverses
            if new_c or new_r:
                combos |= new_c
                reverses |= new_r
                record(f"reds_all_s{seed}", "REDS", seed)
            seed += 1
            assert seed < 200 and before <= (len(combos), len(reverses))
        assert len(combos) == 8 and reverses == {False, True}
        record("reds_mirrors", "REDS", 101, use_mirrors=True)
        record("reds_no_reverse", "REDS", 102, random_reverse=False)
        record("reds_no_hflip", "REDS", 103, use_hflip=False)
        record("reds_no_vflip", "REDS", 104, use_vflip=False)
        record("reds_no_rot", "REDS", 105, use_rot=False)
        record("reds_pre_seed", "REDS", 106, pre_seed=7)
        record("reds_pre_seed_mirrors", "REDS", 107, pre_seed=11, use_mirrors=True, use_vflip=False)
        record("reds_big_crop", "REDS", 108, crop_size=32, use_rot=False)       # 8 > 6 LR rows: clipped to 6 x 8 / 24 x 32
        record("vimeo_all", "Vimeo", 109, num_frames=5)
        record("vimeo_mirrors_no_hflip", "Vimeo", 110, num_frames=5, use_mirrors=True, use_hflip=False)
        record("vimeo_pre_seed", "Vimeo", 111, num_frames=5, pre_seed=3)           # numpy's stream is seeded but never drawn from

    meta = {
        "cases": cases, "scale": SCALE, "keys": KEYS,
        "values": "hr / lr: (clips, frames, H, W, 3) uint8 in the store's B, G, R order; <case>/LRs, <case>/HRs: the stacked 'LRs' / 'HRs' of "
                  "dataset[i] for i in the case's indices, float32, after random.seed(seed) and a freshly constructed dataset (rank 0)",
        "source": "REDSDataset / VimeoDataset of the reference's data/REDS.py and data/Vimeo.py, imported unmodified",
    }
    data["meta"] = np.array(json.dumps(meta))
    path = os.path.join(ROOT, "tests", "golden", "train_batches.npz")
    np.savez_compressed(path, **data)
    print("wrote", path, os.path.getsize(path), "bytes;", len(cases), "cases")


if __name__ == "__main__":
    main()
