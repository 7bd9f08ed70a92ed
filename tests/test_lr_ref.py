"""tests/lr_ref.py (the float64 restatement of the reference's antialiased bicubic downscale) against the reference's own outputs
(tests/golden/lr_bicubic.npz, written by tools/gen_lr_golden.py from utils/image_resize.py imresize_np), and the properties that pin
its three ingredients: the mirror rule, the 0.5 (1 - s) offset, the normalisation.  No GPU.

Bound: every value within 1e-3 on the 0..255 scale of the reference's float32 output -- two passes of <= 18 float32 products of
magnitude <= ~330 with float32 weights give a worst case of about 6e-4; measured here: 4.8e-5 (edges x3).
"""
import numpy as np
import pytest

from tests import lr_cases as C
from tests import lr_ref as R

TOL_VS_REFERENCE = 1e-3
FIXTURE_CASES = [tuple(c) for c in C.fixture()[0]["cases"]]


def _worst_vs_fixture(down):
    _, z = C.fixture()
    return max(float(np.abs(down(z[n + "/hr"], s) - z[f"{n}/x{s}"].astype(np.float64)).max()) for n, s in FIXTURE_CASES)


@pytest.mark.parametrize("name,s", FIXTURE_CASES)
def test_restatement_matches_the_reference_outputs(name, s):
    _, z = C.fixture()
    hr, want = z[name + "/hr"], z[f"{name}/x{s}"]
    assert hr.dtype == np.uint8 and want.dtype == np.float32 and hr.shape[0] <= 64 and hr.shape[1] <= 96
    got = R.bicubic_down(hr, s)
    assert got.dtype == np.float64 and got.shape == want.shape == (hr.shape[0] // s, hr.shape[1] // s, 3)
    d = float(np.abs(got - want.astype(np.float64)).max())
    print(f"{name} x{s}: max |restatement - reference| = {d:.3e}")
    assert d <= TOL_VS_REFERENCE


def test_fixture_covers_the_scales_and_the_clamp():
    meta, z = C.fixture()
    assert {s for _, s in FIXTURE_CASES} == {2, 3, 4}
    for name, s in FIXTURE_CASES:
        want = z[f"{name}/x{s}"].astype(np.float64)
        share = float(np.mean(R.half_integer_distance(want) <= meta["half_band"]))
        assert share <= 0.01, (name, s, share)  # the byte comparison against the float32 reference may leave out at most 1 % of a case
        if name in meta["clamped"]:
            assert want.min() < -0.5 and want.max() > 255.5, (name, s)
    assert 30 <= z["noise/x4"].min() and z["noise/x4"].max() <= 225  # noise alone never reaches the clamp


@pytest.mark.parametrize("what", ["mirror", "offset", "normalisation"])
def test_a_changed_ingredient_misses_the_reference(what, monkeypatch):
    """Each of the three ingredients, replaced by a plausible other choice, leaves the 1e-3 band by orders of magnitude."""
    assert _worst_vs_fixture(R.bicubic_down) <= TOL_VS_REFERENCE
    if what == "mirror":      # reflect without repeating the edge sample: -1 -> 1
        monkeypatch.setattr(R, "mirror", lambda i, n: -i if i < 0 else (2 * n - 2 - i if i >= n else i))
    elif what == "offset":    # sample centres without the half-pixel term
        def table(s):
            w = np.array([R.cubic((s - (s - 2 * s + p)) / s) for p in range(4 * s + 2)], dtype=np.float64)
            return s - 2 * s - 1, w / w.sum()
        monkeypatch.setattr(R, "weight_table", table)
    else:                     # the raw kernel values, not divided by their sum
        true_table = R.weight_table

        def table(s):
            first, _ = true_table(s)
            u = s + 0.5 * (1 - s)
            return first, np.array([R.cubic((u - (first + 1 + p)) / s) for p in range(4 * s + 2)], dtype=np.float64)
        monkeypatch.setattr(R, "weight_table", table)
    worst = _worst_vs_fixture(R.bicubic_down)
    print(f"{what} changed: max |restatement - reference| = {worst:.3e}")
    assert worst > 100 * TOL_VS_REFERENCE


@pytest.mark.parametrize("s", [2, 3, 4])
def test_weight_table(s):
    first, w = R.weight_table(s)
    assert len(w) == 4 * s + 2 and w[0] == 0.0 and w[-1] == 0.0   # the two end entries carry nothing
    assert abs(w.sum() - 1.0) <= 1e-15
    assert first == {2: -4, 3: -5, 4: -7}[s]
    centre = s + 0.5 * (1 - s) - 1          # 0-based position of output 0
    pos = first + np.arange(len(w))
    assert abs(float((w * pos).sum()) - centre) <= 1e-12           # the filter does not shift the image


@pytest.mark.parametrize("s", [2, 3, 4])
def test_flat_frame_stays_flat(s):
    got = R.bicubic_down(np.full((12 * s, 16 * s, 3), 255, np.uint8), s)
    assert float(np.abs(got - 255.0).max()) <= 1e-10


@pytest.mark.parametrize("s", [2, 3, 4])
def test_corner_impulses_give_the_outer_product_of_the_table(s):
    """One pixel of value 1 in a corner: output (oy, ox) is the product of the weights with which rows oy and columns ox reach that
    pixel, directly or through the mirror (written out here with explicit loops, not through axis_matrix)."""
    H, W = 8 * s, 12 * s
    first, w = R.weight_table(s)

    def reach(o, target, n):
        return sum(wp for p, wp in enumerate(w) if R.mirror(o * s + first + p, n) == target)

    for cy, cx in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        img = np.zeros((H, W))
        img[cy, cx] = 1.0
        got = R.bicubic_down(img, s)
        want = np.outer([reach(o, cy, H) for o in range(H // s)], [reach(o, cx, W) for o in range(W // s)])
        assert float(np.abs(got - want).max()) <= 1e-15
        assert np.count_nonzero(want) >= 4 and abs(want.sum() - got.sum()) <= 1e-15
    # the first output reaches the corner sample twice, directly and as the mirror image of sample -1
    assert sum(1 for p in range(len(w)) if w[p] != 0.0 and R.mirror(first + p, H) == 0) == 2


def test_rounding_is_half_to_even_with_saturation():
    assert R.to_uint8(np.array([-3.2, -0.5, 0.5, 1.5, 2.5, 254.5, 255.5, 290.0])).tolist() == [0, 0, 0, 2, 2, 254, 255, 255]


@pytest.mark.parametrize("cid", list(C.CASES))
def test_gpu_cases_have_no_rounding_ties(cid):
    """The condition on the inputs of the byte-for-byte GPU tests: no reference value within 1e-9 of a half-integer; and the clamp is
    exercised at both ends."""
    s, hr, ref = C.case(cid)
    assert hr.dtype == np.uint8 and ref.shape == (hr.shape[0], hr.shape[1] // s, hr.shape[2] // s, 3)
    assert float(R.half_integer_distance(ref).min()) > C.TIE_BAND
    assert ref.min() < -0.5 and ref.max() > 255.5
