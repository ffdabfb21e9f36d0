"""Which path a CNBlock takes (the table): mmgclip.networks.convnext_plan against every row of it, for ConvNeXt-T and -B
under the default knobs and under each of the knobs listed below the table.  No GPU and no kernel library: what the library supports is
passed in as the literal below (csrc/cnblock_mlp.hip: mmg_cnblock_mlp_bwd_supported and the forward's dispatch; csrc/cnblock_bwdw.hip:
mmg_cnblock_bwdw_supported; mmgclip.kernels.cnblock_bwdw_supported for the row-count rule)."""
import pytest

from mmgclip.networks.convnext import CONFIGS, ConvNextTower
from mmgclip.networks.convnext_plan import Knobs, SaveDecision, Support, decide_saves, fused_forward, plan_block, saving_form

FUSED_FWD = (96, 128, 192, 256, 384, 512)
FUSED_BWD_MODE = {96: 1, 128: 1, 192: 1, 384: 2}
SUPPORT = Support(fused_fwd=lambda C: C in FUSED_FWD, fused_bwd_mode=lambda C: FUSED_BWD_MODE.get(C, 0),
                  bwdw=lambda C, M: C == 96 and M % 64 == 0 and 2 * M * C < 2 ** 32)
ALL = SaveDecision(True, True, True)         # every optional tensor fits
NONE = SaveDecision(False, False, False)
M = 64 * 24                                  # rows of a micro-batch: a multiple of 64


def paths(variant, knobs=Knobs(), dec=ALL, rows=M, save_dgelu=True):
    """{C: (forward of a saving pass, forward of a pass that saves nothing, backward, 4C-wide tensor kept, LN output kept, GELU kept)}"""
    out = {}
    for C in CONFIGS[variant]["dims"]:
        p = plan_block(C, knobs, SUPPORT)
        fwd = ["fp8" if p.kind == "fp8" else ("fused" if fused_forward(p, save) else "gemm") for save in (True, False)]
        out[C] = (fwd[0], fwd[1]) + saving_form(p, dec, rows, save_dgelu, SUPPORT)
    return out


def test_default_paths_of_convnext_tiny():
    assert paths("tiny") == {96: ("fused", "fused", "bwdw", None, False, False),          # nothing 4C-wide kept: recomputed on chip
                             192: ("fused", "fused", "fused", None, False, False),
                             384: ("fused", "fused", "gemm", "dgelu", True, True),
                             768: ("gemm", "gemm", "gemm", "dgelu", True, True)}
    # what the GEMM-pair backwards get follows the forward's decision: h and GELU' are alternatives in the same bytes
    assert paths("tiny", dec=NONE)[384] == ("fused", "fused", "gemm", "h", False, False)
    assert paths("tiny", dec=SaveDecision(True, False, False))[768] == ("gemm", "gemm", "gemm", "h", True, False)
    assert paths("tiny", dec=SaveDecision(False, True, False))[384] == ("fused", "fused", "gemm", "dgelu", False, True)
    assert paths("tiny", save_dgelu=False)[384] == ("fused", "fused", "gemm", "h", True, True)
    assert paths("tiny", dec=NONE)[96] == paths("tiny")[96] and paths("tiny", dec=NONE)[192] == paths("tiny")[192]


@pytest.mark.parametrize("rows,want", [(64, "bwdw"), (64 * 37, "bwdw"), (64 * 37 + 1, "fused"), (25 * 17 * 2, "fused"), (63, "fused"),
                                       (2 ** 32 // (2 * 96) // 64 * 64, "bwdw"), ((2 ** 32 // (2 * 96) // 64 + 1) * 64, "fused")])
def test_stage1_backward_is_chosen_by_the_forward_from_its_row_count(rows, want):
    """C = 96: on-chip weight gradients need M % 64 == 0 and 2 M C < 2^32; the forward knows M and records the choice."""
    assert paths("tiny", rows=rows)[96][2] == want
    assert paths("tiny", rows=rows)[192][2] == "fused"            # (no other width has that kernel)


def test_default_paths_of_convnext_base():
    assert paths("base") == {128: ("fused", "fused", "fused", None, False, False),
                             256: ("fused", "fused", "gemm", "dgelu", True, True),
                             512: ("gemm", "fused", "gemm", "dgelu", True, True),          # fused only when nothing is saved
                             1024: ("gemm", "gemm", "gemm", "dgelu", True, True)}
    assert paths("base", dec=NONE)[512] == ("gemm", "fused", "gemm", "h", False, False)


def test_paths_of_convnext_base_fp8():
    fp8 = Knobs(fp8=True, fp8_min_channels=256)
    now = paths("base", fp8, SaveDecision(True, True, True))
    assert now[128] == paths("base")[128]
    for C in (256, 512, 1024):
        assert now[C] == ("fp8", "fp8", "fp8", "dgelu", True, True)               # GELU' + the e4m3 LayerNorm output / activation
    later = paths("base", fp8, SaveDecision(True, True, False))                   # the 8-bit operands do not fit: bf16 backward on h, both rebuilt
    for C in (256, 512, 1024):
        assert later[C] == ("fp8", "fp8", "gemm", "h", False, False)
    plan = [plan_block(C, fp8, SUPPORT) for C in CONFIGS["base"]["dims"]]
    assert [p.kind for p in plan] == ["fused", "fp8", "fp8", "fp8"] and [p.fp8_bwd_weights for p in plan] == [False, True, True, True]
    # C % 128 == 0 is part of the rule: ConvNeXt-T's 96 and 192 never qualify
    assert [plan_block(C, Knobs(fp8=True, fp8_min_channels=96), SUPPORT).kind for C in CONFIGS["tiny"]["dims"]] == ["fused", "fused", "fp8", "fp8"]


def test_knob_bwdw_off_removes_the_on_chip_weight_gradients():
    off = paths("tiny", Knobs(bwdw=False))
    assert off[96] == ("fused", "fused", "fused", None, False, False)
    assert {C: v for C, v in off.items() if C != 96} == {C: v for C, v in paths("tiny").items() if C != 96}
    assert not any(plan_block(C, Knobs(bwdw=False), SUPPORT).bwdw for C in CONFIGS["tiny"]["dims"])
    assert [plan_block(C, Knobs(), SUPPORT).bwdw for C in CONFIGS["tiny"]["dims"]] == [True, False, False, False]


@pytest.mark.parametrize("variant", ["tiny", "base"])
def test_knob_fused_mlp_off_turns_every_fused_row_into_a_gemm_pair(variant):
    for C, row in paths(variant, Knobs(fused_mlp=False)).items():
        assert row == ("gemm", "gemm", "gemm", "dgelu", True, True), C


def test_knob_saved_h_makes_the_384_backward_fused():
    on = paths("tiny", Knobs(fused_bwd_saved_h=True))
    assert on[384] == ("fused", "fused", "fused", "h", False, False)              # mode 2 reads the forward's pre-activation
    assert {C: v for C, v in on.items() if C != 384} == {C: v for C, v in paths("tiny").items() if C != 384}
    assert [plan_block(C, Knobs(fused_bwd_saved_h=True), SUPPORT).fused_bwd for C in CONFIGS["tiny"]["dims"]] == [1, 1, 2, 0]
    assert [plan_block(C, Knobs(), SUPPORT).fused_bwd for C in CONFIGS["base"]["dims"]] == [1, 0, 0, 0]


def test_knob_fp8_bwd_off_moves_the_threshold_to_512_and_removes_the_8_bit_backward(monkeypatch):
    monkeypatch.setenv("MMG_FP8_BWD", "0")
    monkeypatch.delenv("MMG_FP8_MIN_C", raising=False)
    tower = ConvNextTower("base", fp8=True)
    knobs = tower.knobs()
    assert (knobs.fp8_min_channels, knobs.fp8_bwd, tower.fp8_bwd) == (512, False, False)
    got = paths("base", knobs, ALL)                 # (whatever a decision says: these blocks hold no 8-bit backward weights)
    assert got[256] == paths("base")[256]
    assert got[512] == got[1024] == ("fp8", "fp8", "gemm", "h", False, False)
    plan = [plan_block(C, knobs, SUPPORT) for C in tower.dims]
    big = [(256, 1024, 1024)]
    assert decide_saves(plan, tower.depths, [(1, 64, 64)], 288 << 30, fp8_bwd=tower.fp8_bwd_mode).fp8_bwd_now is False
    monkeypatch.delenv("MMG_FP8_BWD")
    tower = ConvNextTower("base", fp8=True)
    assert (tower.knobs().fp8_min_channels, tower.fp8_bwd, tower.fp8_bwd_mode) == (256, True, "auto")
    plan = [plan_block(C, tower.knobs(), SUPPORT) for C in tower.dims]
    # MMG_FP8_BWD: 0 off, 1 always, anything else by memory
    assert decide_saves(plan, tower.depths, [(1, 64, 64)], 288 << 30, fp8_bwd="auto").fp8_bwd_now is True
    assert decide_saves(plan, tower.depths, big, 288 << 30, fp8_bwd="auto").fp8_bwd_now is False
    assert decide_saves(plan, tower.depths, big, 288 << 30, fp8_bwd="1").fp8_bwd_now is True
    assert decide_saves(plan, tower.depths, [(1, 64, 64)], 288 << 30, fp8_bwd="0").fp8_bwd_now is False


def test_knob_fused_save_maxc_moves_saving_forwards_to_the_gemm_pair():
    """MMG_MLP_FUSED_SAVE_MAXC (A/B knob): beyond it a fused block's SAVING forward is the GEMM pair, and so is its backward then."""
    got = paths("tiny", Knobs(fused_save_maxc=192))
    assert got[384] == ("gemm", "fused", "gemm", "dgelu", True, True) and got[192] == paths("tiny")[192]
    assert paths("tiny", Knobs(fused_save_maxc=0))[96] == ("gemm", "fused", "gemm", "dgelu", True, True)


def test_save_decision_thresholds_and_byte_counts():
    """decide_saves on a 288 GiB device (MI355X): the byte counts behind tests/test_configs_gpu.py::test_saved_layernorm_output_is_bounded_by_device_memory
    (ConvNeXt-T at 256 x 1024^2: LayerNorm outputs of the 12 GEMM-pair blocks 8.4 GB)."""
    total = 288 << 30
    tiny = [plan_block(C, Knobs(), SUPPORT) for C in CONFIGS["tiny"]["dims"]]
    base = [plan_block(C, Knobs(), SUPPORT) for C in CONFIGS["base"]["dims"]]
    td, bd = CONFIGS["tiny"]["depths"], CONFIGS["base"]["depths"]
    ln_bytes = 256 * 2 * (9 * 64 * 64 * 384 + 3 * 32 * 32 * 768)
    assert ln_bytes == 8455716864
    # at the share (a few bytes of slack for the float product): kept; just below it: not
    assert decide_saves(tiny, td, [(256, 1024, 1024)], ln_bytes / 0.04 + 64).save_ln is True
    assert decide_saves(tiny, td, [(256, 1024, 1024)], ln_bytes / 0.04 - 64).save_ln is False
    assert decide_saves(tiny, td, [(256, 1024, 1024)], 4 * ln_bytes / 0.15 - 64) == SaveDecision(True, False, False)
    assert decide_saves(tiny, td, [(256, 1024, 1024)], total) == SaveDecision(True, True, False)
    assert decide_saves(base, bd, [(256, 1024, 1024)], total) == SaveDecision(False, False, False)
    assert decide_saves(base, bd, [(64, 1024, 1024)], total).save_ln is True
    assert decide_saves(base, bd, [(128, 1024, 1024)], total) == SaveDecision(False, False, False)
    assert decide_saves(base, bd, [(128, 1024, 1024)], total, ckpt=True) == SaveDecision(True, True, False)
    assert decide_saves(base, bd, [(256, 1024, 1024)], total, ckpt=True).save_gelu is False
    # several image sizes alive at once add up; odd maps floor at every stride
    one = decide_saves(tiny, td, [(1, 77, 50)], 1).save_ln
    assert one is False and decide_saves(tiny, td, [(1, 77, 50)], 2 * (9 * 4 * 3 * 384 + 3 * 2 * 1 * 768) / 0.04 + 64).save_ln is True
    assert decide_saves(tiny, td, [(128, 1024, 1024), (128, 1024, 1024)], ln_bytes / 0.04 + 64).save_ln is True
    assert decide_saves(tiny, td, [(128, 1024, 1024), (129, 1024, 1024)], ln_bytes / 0.04).save_ln is False
    # forced modes
    assert decide_saves(base, bd, [(256, 1024, 1024)], total, save_ln="1", save_gelu="1") == SaveDecision(True, True, False)
    assert decide_saves(tiny, td, [(1, 64, 64)], total, save_ln="0", save_gelu="0") == SaveDecision(False, False, False)
