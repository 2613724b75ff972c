"""Host only (needs hipcc, no GPU): the generated gfx950 code of csrc/convs16.hip keeps the 27-tap weights where its MFMAs read them.

The depth-walking forms hold 216 weight registers per wave.  Left to itself the register allocator parks fragments in AGPRs and copies each
back with four v_accvgpr_read_b32 in front of its MFMA, every step: 11 to 37 copies per steady-state step in the forms without the fused head,
117 in the head form.  With the weights declared AGPR values the MFMAs take srcA from the AGPRs and the copies go away (1.6 per
step; 14.6 in the head form, whose product P leaves the accumulator through VGPRs).  tools/isa_step_stats.py counts them in the compiler's
assembly; the caps sit between the two: at most 8 copies per step without the head, 32 with it, and no form spills or touches scratch."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("isa_step_stats", os.path.join(ROOT, "tools", "isa_step_stats.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def kernels():
    tool = _tool()
    if not os.path.exists(tool.B.HIPCC):
        pytest.skip("hipcc missing")
    ks = [k for k in tool.stats("convs16.hip", "convs16_kernel<") if not k["name"].split("<")[1].split(",")[1] == "true"]     # (CV: s16_cvrows.h, no depth walk)
    assert len(ks) >= 12 and all(k["steps"] >= 6 for k in ks), "every depth-walking form has its steady-state steps between barriers"
    return ks


def test_no_form_spills_or_uses_scratch(kernels):
    for k in kernels:
        assert (k["vgpr_spills"], k["scratch_bytes"], k["scratch_insts"]) == (0, 0, 0), k["name"]
        assert k["agprs"] <= 256 and k["vgprs"] <= 512, k["name"]


def test_steady_state_steps_do_not_copy_weights_back_from_agprs(kernels):
    heads = [k for k in kernels if k["name"].endswith(",true>")]
    assert len(heads) == 1
    for k in kernels:
        cap = 32 if k in heads else 8
        print(f"{k['name']}: {k['per_step']['copies']:.1f} v_accvgpr_* per step, {k['per_step']['mfma_srca_agpr']:.1f} of {k['per_step']['mfma']:.1f} MFMAs read srcA from AGPRs")
        assert k["per_step"]["copies"] <= cap, k["name"]
        assert 54 <= k["per_step"]["mfma"] <= 84, k["name"]                 # (the steps counted are depth steps: 54 to 84 MFMAs each)
