"""The numpy restatement of what the reference's dataset classes do to stored frames once the random numbers are drawn
(data/REDS.py:166-215, data/Vimeo.py:159-206): slow and obvious, one frame and one step at a time.  TEST INFRASTRUCTURE.

    sample(hr_clip, lr_clip, frames, y0, x0, hflip, vflip, rot, crop, scale, bgr=True) -> (LRs (T', 3, h, w), HRs (T', 3, s h, s w)) float32
    batch(hr, lr, plan, scale, bgr=True) -> the stacked samples of a vmg_amd.batches.BatchPlan
hr_clip / lr_clip: (F, H, W, 3) uint8 arrays in the store's channel order; frames: the frame indices in output order (mirrors included).
"""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_batches.npz")


def read_img(frame_u8):
    return frame_u8.astype(np.float32) / 255.   # a true division, data/REDS.py:116


def augment(img, hflip, vflip, rot):
    if hflip:
        img = img[:, ::-1, :]
    if vflip:
        img = img[::-1, :, :]
    if rot:
        img = img.transpose(1, 0, 2)
    return img


def sample(hr_clip, lr_clip, frames, y0, x0, hflip, vflip, rot, crop, scale, bgr=True, as_bytes=False):
    outs = []
    for clip, m in ((lr_clip, 1), (hr_clip, scale)):
        imgs = []
        for f in frames:
            img = clip[f] if as_bytes else read_img(clip[f])
            img = img[m * y0:m * y0 + m * crop, m * x0:m * x0 + m * crop, :]   # slicing clips a crop larger than the frame
            img = augment(img, hflip, vflip, rot)
            if bgr:
                img = img[:, :, [2, 1, 0]]
            imgs.append(np.transpose(img, (2, 0, 1)))
        outs.append(np.ascontiguousarray(np.stack(imgs, axis=0)))
    return outs[0], outs[1]


def batch(hr, lr, plan, scale, bgr=True, as_bytes=False):
    """hr / lr: indexable by clip, each clip (F, H, W, 3) uint8."""
    pairs = [sample(hr[int(plan.clip[b])], lr[int(plan.clip[b])], [int(f) for f in plan.frames[b]], int(plan.y0[b]), int(plan.x0[b]),
                    bool(plan.hflip[b]), bool(plan.vflip[b]), bool(plan.rot[b]), int(plan.crop), scale, bgr, as_bytes) for b in range(len(plan.clip))]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


_fixture = None


def fixture():
    """(meta, arrays) of tests/golden/train_batches.npz, loaded once and shared; the arrays are read-only."""
    global _fixture
    if _fixture is None:
        z = np.load(GOLDEN)
        arrays = {k: z[k] for k in z.files if k != "meta"}
        for a in arrays.values():
            a.setflags(write=False)
        _fixture = (json.loads(str(z["meta"])), arrays)
    return _fixture


def case_rngs(case):
    """The generators a fixture case was recorded with: random.seed(seed) and, with pre_seed, numpy seeded pre_seed + rank + 1 (rank 0)."""
    import random
    pre = case["cfg"]["pre_seed"]
    return random.Random(case["seed"]), (np.random.RandomState(pre + 0 + 1) if pre is not None else None)
