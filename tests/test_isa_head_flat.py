"""Host only (needs hipcc, no GPU): the generated gfx950 code of the fused head on flat tiles, csrc/convs16.hip's convs16_headflat_kernel
(DESIGN 3.18), held to what tests/test_isa_weights_in_agprs.py holds the row head to.  That test counts exactly one fused-head instantiation of
convs16_kernel, so the flat head carries a name of its own and is checked here: no VGPR spill, no scratch, at most 512 VGPRs of which at most
256 AGPRs, at most 32 v_accvgpr_* copies per steady-state step (the product P leaving its accumulator, not weights coming back), and depth
steps of 54 to 84 MFMAs.  The other instantiations of the file must still be the nineteen depth-walking forms plus the cost-volume one."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("isa_step_stats", os.path.join(ROOT, "tools", "isa_step_stats.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    if not os.path.exists(mod.B.HIPCC):
        pytest.skip("hipcc missing")
    return mod


def test_flat_head_keeps_the_row_heads_register_budget(tool):
    ks = tool.stats("convs16.hip", "convs16_headflat_kernel<")
    assert [k["name"] for k in ks] == ["convs16_headflat_kernel<2,false,0,28,false,false,true>"]
    k = ks[0]
    print(f"{k['name']}: {k['vgprs']} VGPRs ({k['agprs']} AGPRs), {k['per_step']['copies']:.1f} v_accvgpr_* and {k['per_step']['mfma']:.1f} MFMAs per step")
    assert k["steps"] >= 6
    assert (k["vgpr_spills"], k["scratch_bytes"], k["scratch_insts"]) == (0, 0, 0)
    assert k["agprs"] <= 256 and k["vgprs"] <= 512
    assert k["per_step"]["copies"] <= 32
    assert 54 <= k["per_step"]["mfma"] <= 84
