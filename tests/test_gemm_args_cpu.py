"""Argument validation of the five GEMM entry points (no GPU): every call below must be rejected before any HIP call, with a message
that starts with the name of the entry point that was called.  No call here is a valid one, so none reaches a launch."""
import pytest

from mmgclip import _hip

PTR = 0x1000            # stands for a device pointer: validation compares pointers with NULL and never dereferences them
M, N = 256, 128
OPTIONAL = ("bias", "colscale", "residual", "aux_in", "aux_out", "alpha_dev", "alpha_dev2", "colsum_a", "stream")

# NT entry point -> (K, alignment of lda / ldb, epilogues it does not have, epilogues that need aux_in, out kinds it does not have)
NT_DOORS = {
    "mmg_gemm_nt_bf16": (64, 8, (-1, 8), (2, 4, 5, 7), ()),
    "mmg_gemm_nt_fp8": (128, 16, (-1, 2, 4, 5, 7, 8), (), (-1, 3)),
    "mmg_gemm_nt_fp8_bwd": (128, 16, (-1, 1, 2, 3, 4, 6, 8), (5, 7), (-1, 2, 4)),
}
# TN entry point -> alignment of N1 / N2 / lda / ldb (and their minimum)
TN_DOORS = {"mmg_gemm_tn_bf16": 8, "mmg_gemm_tn_fp8": 16}
N1, N2 = 128, 256


def _cases():
    protos = _hip.parse_header()
    for name, (K, lda_al, no_epi, aux_epi, no_out) in NT_DOORS.items():
        names = protos[name][2]
        valid = {"lda": K, "ldb": K, "ldc": N, "ldr": N, "ldai": N, "ldao": N, "M": M, "N": N, "K": K, "epi": 0, "out_f32": 0, "out_kind": 0,
                 "a_e5m2": 1, "alpha": 1.0}
        bad = [("A_null", {"A": None}), ("B_null", {"B": None}), ("C_null", {"C": None}),
               ("M_zero", {"M": 0}), ("N_zero", {"N": 0}), ("K_zero", {"K": 0}), ("M_negative", {"M": -256}), ("N_negative", {"N": -128}),
               ("K_unaligned", {"K": K - K // 4, "lda": K, "ldb": K}),              # 48 (not a multiple of 32) / 96 (not of 128)
               ("N_unaligned", {"N": N + 4, "ldc": N + 8, "ldr": N + 8, "ldai": N + 8, "ldao": N + 8}),
               ("lda_small", {"lda": K - lda_al}), ("ldb_small", {"ldb": K - lda_al}), ("ldc_small", {"ldc": N - 8}),
               ("lda_unaligned", {"lda": K + lda_al // 2}), ("ldb_unaligned", {"ldb": K + lda_al // 2}), ("ldc_unaligned", {"ldc": N + 4})]
        bad += [(f"epi_{e}_unavailable", {"epi": e, "aux_in": PTR}) for e in no_epi]
        for e in aux_epi:
            bad += [(f"epi_{e}_aux_in_null", {"epi": e, "aux_in": None}), (f"epi_{e}_ldai_small", {"epi": e, "aux_in": PTR, "ldai": N - 8}),
                    (f"epi_{e}_ldai_unaligned", {"epi": e, "aux_in": PTR, "ldai": N + 4})]
        if "residual" in names:
            bad += [("ldr_small", {"residual": PTR, "ldr": N - 8}), ("ldr_unaligned", {"residual": PTR, "ldr": N + 4})]
        if "aux_out" in names:
            bad += [("ldao_small", {"aux_out": PTR, "ldao": N - 8}), ("ldao_unaligned", {"aux_out": PTR, "ldao": N + 4})]
        bad += [(f"out_kind_{k}", {"out_kind": k}) for k in no_out]
        for label, override in bad:
            yield pytest.param(name, _args(names, valid, override), id=f"{name}-{label}")
    for name, al in TN_DOORS.items():
        names = protos[name][2]
        valid = {"lda": N1, "ldb": N2, "ldc": N2, "M": M, "N1": N1, "N2": N2, "a_e5m2": 1, "alpha": 1.0}
        bad = [("A_null", {"A": None}), ("B_null", {"B": None}), ("C_null", {"C": None}), ("M_zero", {"M": 0}), ("M_negative", {"M": -64}),
               ("N1_zero", {"N1": 0}), ("N2_below_minimum", {"N2": al // 2}), ("N1_unaligned", {"N1": N1 + al // 2, "lda": N1 + al}),
               ("N2_unaligned", {"N2": N2 + al // 2, "ldb": N2 + al, "ldc": N2 + al}), ("lda_small", {"lda": N1 - al}), ("ldb_small", {"ldb": N2 - al}),
               ("ldc_small", {"ldc": N2 - 8}), ("lda_unaligned", {"lda": N1 + al // 2}), ("ldb_unaligned", {"ldb": N2 + al // 2})]
        for label, override in bad:
            yield pytest.param(name, _args(names, valid, override), id=f"{name}-{label}")


def _args(names, valid, override):                       # (an override of an argument the entry point does not have is dropped)
    return [override[n] if n in override else valid[n] if n in valid else None if n in OPTIONAL else PTR for n in names]


@pytest.mark.parametrize("name,args", list(_cases()))
def test_gemm_rejects_bad_arguments(name, args):
    lib = _hip.load()
    rc = getattr(lib, name)(*args)
    assert rc != 0
    message = lib.mmg_last_error().decode()
    assert message.startswith(name + ":"), message
    assert "launch failed" not in message, message          # rejected by validation, not by a launch that went wrong
