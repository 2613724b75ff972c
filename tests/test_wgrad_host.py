"""CPU checks behind tests/test_hip_wgrad_edges.py: the fp64 reference of tests/wgrad_oracle.py equals torch autograd, every branch of
csrc/wgrad.hip and csrc/wgrad_slide.hip the GPU module is there for is reached by a named case (according to the launch model), every
plausible kernel mistake that applies to a case is visible in it, and no launch -- the cases' and every weight-gradient launch of the
Config-A and Config-B train steps -- reads past the over-read room behind a blocked tensor."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import wgrad_oracle as O


# ------------------------------------------------------------------------------------------------ reference == autograd
AUTOGRAD = [
    O.conv_case("c3 s1 odd", 2, 5, 7, (3, 5, 7), 3),
    O.conv_case("c3 s1 even", 2, 6, 4, (4, 6, 8), 3),
    O.conv_case("c3 s2 odd", 2, 5, 7, (5, 7, 9), 3, stride=2),
    O.conv_case("c3 s2 even", 2, 6, 4, (4, 6, 8), 3, stride=2),
    O.deconv_case("up odd", 2, 5, 7, (3, 5, 7)),
    O.deconv_case("up even", 2, 6, 4, (2, 4, 6)),
    O.conv_case("2d k3", 2, 5, 7, (1, 9, 13), (1, 3, 3)),
    O.conv_case("2d k3 halo 2", 2, 5, 7, (1, 9, 13), (1, 3, 3), halo=(0, 2, 2)),
    O.conv_case("2d k3 dil 2", 2, 5, 7, (1, 9, 13), (1, 3, 3), dil=2),
    O.conv_case("2d k3 dil 4", 2, 5, 7, (1, 9, 13), (1, 3, 3), dil=4),
    O.conv_case("2d k3 dil 4 small", 2, 5, 7, (1, 3, 13), (1, 3, 3), dil=4),
    O.conv_case("2d k3 s2 odd", 2, 5, 7, (1, 11, 15), (1, 3, 3), stride=2),
    O.conv_case("2d k3 s2 even", 2, 5, 7, (1, 10, 14), (1, 3, 3), stride=2),
    O.conv_case("2d k1", 2, 5, 7, (1, 10, 14), (1, 1, 1), halo=(0, 1, 1)),
    O.conv_case("2d k1 s2", 2, 5, 7, (1, 9, 13), (1, 1, 1), stride=2, halo=(0, 1, 1)),
    O.conv_case("2d k7 s2 p3", 2, 3, 7, (1, 14, 18), (1, 7, 7), stride=2),
]


def _autograd(case, a, b):
    """weight.grad of the layer behind a case, as the kernel's [Ca][Cb][T]"""
    a, b = torch.from_numpy(a).double(), torch.from_numpy(b).double()
    conv = case["conv"]
    if conv["kind"] == "deconv":                                          # a = dy, b = x; weight [Cin, Cout, k] -> gw[co][ci][k]
        w = torch.zeros(case["Cb"], case["Ca"], 3, 3, 3, dtype=torch.float64, requires_grad=True)
        F.conv_transpose3d(b, w, None, 2, 1, 1).backward(a)
    else:
        w = torch.zeros(case["Cb"], case["Ca"], *conv["k"], dtype=torch.float64, requires_grad=True)
        F.conv3d(a, w, None, conv["stride"], conv["pad"], conv["dil"]).backward(b)
    return w.grad.permute(1, 0, 2, 3, 4).reshape(case["Ca"], case["Cb"], -1).numpy()


@pytest.mark.parametrize("case", AUTOGRAD + [c for c in O.ALL_CASES if c["conv"]], ids=lambda c: c["name"])
def test_reference_is_autograd(case):
    a = O.hash_uniform(f"ag:{case['name']}:a", (case["N"], case["Ca"]) + case["a_dims"]).numpy()
    b = O.hash_uniform(f"ag:{case['name']}:b", (case["N"], case["Cb"]) + case["b_dims"]).numpy()
    gw, mag, terms = O.reference(O.pad_a(case, a), b, case["cls"], case["in_mul"])
    ref = _autograd(case, a, b)
    assert gw.shape == ref.shape and np.abs(ref).max() > 0.1
    assert np.abs(gw - ref).max() <= 1e-12 * np.abs(ref).max()
    assert (mag >= np.abs(gw)).all() and (terms == case["N"] * int(np.prod(case["b_dims"]))).all()


def test_reference_formula_by_hand():
    """the header's formula written as loops, on a tap class no layer has (2 x 1 x 2 taps, in_mul 2, first (1, 0, 1), step (1, 1, 2))"""
    cls = dict(n=(2, 1, 2), first=(1, 0, 1), step=(1, 1, 2))
    a = O.hash_uniform("hand:a", (2, 3, 7, 5, 9)).numpy().astype(np.float64)
    b = O.hash_uniform("hand:b", (2, 2, 3, 3, 3)).numpy().astype(np.float64)
    gw, _, _ = O.reference(a, b, cls, 2)
    want = np.zeros_like(gw)
    for td in range(2):
        for tw in range(2):
            for n in range(2):
                for od in range(3):
                    for oh in range(3):
                        for ow in range(3):
                            want[:, :, td * 2 + tw] += np.outer(a[n, :, 2 * od + 1 + td, 2 * oh, 2 * ow + 1 + 2 * tw], b[n, :, od, oh, ow])
    assert np.abs(gw - want).max() <= 1e-13


# ------------------------------------------------------------------------------------------------ the cases reach their branches
def test_slide_cases_reach_their_branches():
    m = {c["name"]: O.model_of(c) for c in O.SLIDE_CASES}
    assert all(m[f"S{i}"]["path"] == "slide" and m[f"S{i}"]["partial"] for i in range(1, 11))
    assert (m["S1"]["R"], m["S1"]["WT"], m["S1"]["NK"], m["S1"]["nk"]) == (1, 1, 0, 1) and m["S1"]["idle"] == 3
    assert m["S2"]["R"] * m["S2"]["WT"] == 15 and m["S2"]["NK"] == 0 and m["S2"]["nk"] == 4
    assert m["S3"]["NK"] == 13 and m["S3"]["R"] * m["S3"]["WT"] == 49
    assert m["S4"]["NK"] == 14 and m["S4"]["R"] == 4 and m["S4"]["ragged_rows"]
    assert m["S5"]["NK"] == 16 and (m["S5"]["nseg"], m["S5"]["seglen"], m["S5"]["last_seg"]) == (2, 3, 2)
    assert m["S6"]["WT"] == 17 and m["S6"]["n_wt"] == 2 and m["S6"]["ragged_cols"] and m["S6"]["ragged_rows"]
    assert (m["S6"]["nseg"], m["S6"]["seglen"], m["S6"]["last_seg"]) == (3, 3, 1)
    assert m["S7"]["NK"] == 0 and m["S7"]["nk"] == 15 and m["S7"]["ragged_rows"] and m["S7"]["nseg"] == 3
    assert (m["S8"]["nseg"], m["S8"]["seglen"], m["S8"]["last_seg"]) == (4, 4, 1)
    assert (m["S9"]["units"], m["S9"]["waves"], m["S9"]["per_wave"]) == (126, 64, 2)
    assert O.BY_NAME["S10"]["Ca"] % 16 and O.BY_NAME["S10"]["Cb"] % 16
    assert {m[k]["NK"] for k in m if m[k]["path"] == "slide"} == {0, 13, 14, 16}
    assert {m[k]["nk"] & 1 for k in m if m[k]["path"] == "slide" and m[k]["NK"] == 0} == {0, 1}      # the end-of-tap fetch on either side
    assert m["S11"]["path"] == "generic" and m["S11"]["NT"] == 9 and O.BY_NAME["S11"]["cls"]["n"][0] == 3
    # the atomicAdd flush of the slide kernel: no scratch
    assert not O.model_of(O.BY_NAME["S6"], scratch_floats=0)["partial"]


def test_generic_cases_reach_their_branches():
    m = {c["name"]: O.model_of(c) for c in O.GENERIC_CASES + O.FORCED_CASES + [O.G8, O.G9] + O.RAW_CASES}
    assert all(v["path"] == "generic" for v in m.values())
    assert O.model_of(O.G9S)["path"] == "slide"
    odd = O.BY_NAME["G1odd"]
    assert all(d & 1 for d in odd["a_dims"]) and odd["in_mul"] == 2 and not any(d & 1 for d in O.BY_NAME["G1even"]["a_dims"])
    assert O.BY_NAME["G2a"]["in_mul"] == 2 and O.BY_NAME["G2a"]["conv"]["kind"] == "deconv"
    d4 = O.BY_NAME["G3dil4"]
    assert d4["cls"]["step"][1] == 4 and d4["a_dims"][1] < 2 * 4 + 1                                 # the map is smaller than the dilation span
    assert m["G3k1"]["NT"] == 1 and m["G3k1s2"]["NT"] == 1 and O.BY_NAME["G3k1s2"]["in_mul"] == 2
    assert m["G4"]["jobs"] == 256 and m["G4"]["per_wave"] >= 2 and O.BY_NAME["G4"]["units"] > O.BY_NAME["G4"]["N"]
    assert m["G5"]["ragged_cols"] and "R" not in O.BY_NAME["G5"]                                    # the search's own pick
    assert m["G6"]["ragged_rows"] and m["G6"]["ragged_cols"]
    slots = {k: m[k]["R"] * m[k]["WT"] for k in m if k.startswith("G7")}
    assert {1, 4, 5, 8} <= set(slots.values())
    nms = {m[k]["nm"] for k in m}
    assert {1, 2, 3, 4} <= nms                                   # nm = 1; two steps left at m = 0; loop + one left; loop + two left
    assert any(v["nm"] > 2 and v["nm"] & 1 for v in m.values()) and any(v["nm"] > 2 and not v["nm"] & 1 for v in m.values())
    assert any(v["idle"] for v in m.values())                    # idle waves: their zero partials are read by the reduce
    assert {m[k]["NT"] for k in m} == {1, 2, 4, 9, 49}
    assert (m["NT2"]["NT"], m["NT4"]["NT"], m["NT49"]["NT"]) == (2, 4, 49)
    assert O.BY_NAME["NT49"]["b_dims"] == (1, 7, 9) and O.BY_NAME["NT49"]["in_mul"] == 2


def test_g8_step_down_has_four_outcomes():
    g8 = O.model_of(O.G8)
    assert g8["jobs"] == 192 and g8["groups"] >= 17 and g8["per_wave"] >= 2
    need = g8["need"]
    assert need == [O._ceil(w, 4) * 4 * 192 * 9 * 256 for w in (16, 10, 5)] and need[0] > need[1] > need[2]
    assert need[0] <= O.SCRATCH_FLOATS
    got = [O.model_of(O.G8, scratch_floats=s) for s in (O.SCRATCH_FLOATS, need[0] - 1, need[1] - 1, need[2] - 1)]
    assert [(g["per_simd"], g["waves"], g["partial"]) for g in got] == [(3, 16, True), (2, 12, True), (1, 8, True), (1, 8, False)]
    # overwrite = 0 on both flushes
    assert O.model_of(O.G9)["partial"] and not O.model_of(O.G9, scratch_floats=0)["partial"]


def test_reduce_worker_counts():
    """wgrad_reduce_kernel: four segments of per = ceil(workers / 4) partials, eight at a time and then one by one.  The launchers round the
    worker count up to whole blocks of four waves, so the counts that reach the reduce are multiples of 4: the table has counts that are no
    multiple of 8, runs shorter than 8, runs of exactly 8 and 16, and runs of 8 with a remainder."""
    waves = {O.model_of(c)["waves"] for c in O.ALL_CASES} | {O.model_of(O.G8, scratch_floats=O.model_of(O.G8)["need"][0] - 1)["waves"]}
    assert all(w % 4 == 0 for w in waves)
    assert {4, 12, 20, 36} <= waves
    per = {w // 4 for w in waves}
    assert {1, 2, 3, 5, 8, 16} <= per and any(8 < p < 16 for p in per) and any(p > 16 and p % 8 for p in per)


# ------------------------------------------------------------------------------------------------ sensitivity
@pytest.mark.parametrize("case", O.ALL_CASES, ids=lambda c: c["name"])
def test_every_applicable_mistake_is_visible(case):
    model = O.model_of(case)
    todo = O.mistakes(case, model)
    assert "shift the centre tap by one voxel" in todo or case["a_halo"][2] == 0
    assert ("drop the last row of the ragged tile" in todo) == model["ragged_rows"]
    assert ("skip the last worker" in todo) == model["partial"]
    for kind in ("int", "real"):
        d = O.data(case["name"], kind)
        bound = O.bound(case, model, d["mag"], d["terms"])
        for name, kw in todo.items():
            mut, _, _ = O.reference(O.pad_a(case, d["a"]), d["b"], case["cls"], case["in_mul"], **kw)
            diff = np.abs(mut - d["gw"])
            if kind == "int":
                assert np.array_equal(mut, np.round(mut)) and diff.max() >= 1, name
            else:
                assert (diff / bound).max() >= 10, (name, float((diff / bound).max()))


def test_integer_cases_are_exact_in_fp32():
    """every partial sum of an integer case is an integer below 2^24: fp32 adds them exactly in any order"""
    for c in O.ALL_CASES:
        assert 9 * c["N"] * int(np.prod(c["b_dims"])) < 2 ** 24
        d = O.data(c["name"], "int")
        assert np.abs(d["a"]).max() == 3 and np.abs(d["b"]).max() == 3 and d["mag"].max() < 2 ** 24


# ------------------------------------------------------------------------------------------------ over-read
def test_model_tile_search_is_the_production_one():
    from disprcnn_amd import engine as E
    from disprcnn_amd.modeling.psmnet import train as T
    assert O.SLACK_FLOATS == E.SLACK_FLOATS
    # the picks of the search before it was a function of its own (recorded from wgrad())
    assert T.wgrad_tile_search(28, 28, 1, 2, 2)[:2] == (2, 28)
    assert T.wgrad_tile_search(14, 14, 1, 2, 2)[:2] == (2, 14)
    assert T.wgrad_tile_search(6, 14, 2, 2, 2)[:2] == (6, 14)
    assert T.wgrad_tile_search(56, 56, 1, 4, 4)[:2] == (7, 8)
    for H, W, in_mul, sh, sw in ((28, 28, 1, 2, 2), (17, 35, 1, 2, 2), (7, 9, 2, 6, 6), (3, 13, 1, 8, 8)):
        R, WT, need = T.wgrad_tile_search(H, W, in_mul, sh, sw)
        assert need == T.wgrad_tile_need(R, WT, in_mul, sh, sw) <= T.WGRAD_TILE["lds_max"] and R * WT <= 112


def test_no_launch_reads_past_the_slack():
    """the generic kernel stages its a and b tiles without clamping: a ragged last tile reads on into the following rows, and behind the
    last unit into the slack.  Largest offset read < numel + SLACK_FLOATS, for every case and every layer of Config A and Config B."""
    worst = 0
    for c in O.ALL_CASES:
        m, ga, gb = O.model_of(c), O.geometry(c, "a"), O.geometry(c, "b")
        assert m["a_max"] <= ga["numel"] + O.SLACK_FLOATS and m["b_max"] <= gb["numel"] + O.SLACK_FLOATS, c["name"]
        if m["path"] == "slide":                                 # clamped staging: nothing outside the tensors
            assert m["a_max"] <= ga["numel"] and m["b_max"] <= gb["numel"], c["name"]
    layers = O.psmnet_layers()
    assert len(layers) > 4 * 50
    paths = set()
    for label, c in layers:
        m, ga, gb = O.model_of_layer(c)
        paths.add((m["path"], m["NT"]))
        assert m["a_max"] <= ga["numel"] + O.SLACK_FLOATS and m["b_max"] <= gb["numel"] + O.SLACK_FLOATS, label
        worst = max(worst, m["a_max"] - ga["numel"], m["b_max"] - gb["numel"])
    assert paths == {("slide", 27), ("generic", 9), ("generic", 1)}
    print(f"largest over-read of a Config A / B layer: {worst} floats of {O.SLACK_FLOATS}")
