"""Argument validation of the nine attention entry points (no GPU): every call below must be rejected before any HIP call, with a
message that starts with the name of the entry point that was called.  No call here is a valid one, so none reaches a launch."""
import pytest

from mmgclip import _hip

PTR = 0x1000            # stands for a device pointer: validation compares pointers with NULL and never dereferences them
HEADS, HD = 2, 128

# entry point -> (an S validation must reject, is a backward, is tiled, has dropout arguments)
DOORS = {
    "mmg_attention_fwd": (513, False, False, False),
    "mmg_attention_bwd": (257, True, False, False),
    "mmg_attention_varlen_fwd": (513, False, False, False),
    "mmg_attention_varlen_bwd": (257, True, False, False),
    "mmg_attention_dropout_fwd": (513, False, False, True),
    "mmg_attention_dropout_bwd": (257, True, False, True),
    "mmg_attention_long_fwd": (0, False, True, False),
    "mmg_attention_long_bwd": (0, True, True, False),
    "mmg_attention_dropout_long_bwd": (513, True, True, True),
}
VALID = {"ld": 3 * HD, "ldc": HD, "lddc": HD, "lddq": 3 * HD, "B": 2, "S": 64, "S_max": 64, "heads": HEADS, "Hd": HD, "scale": 0.125,
         "p": 0.1, "seed": 1, "site": 0, "first_sequence": 0, "mask": None, "stream": None}


def _cases():
    protos = _hip.parse_header()
    for name, (bad_s, bwd, tiled, drop) in DOORS.items():
        names = protos[name][2]
        s_name = "S_max" if "S_max" in names else "S"
        bad = [("S", {s_name: bad_s}), ("hidden", {"Hd": HD + 64}), ("ld_unaligned", {"ld": 3 * HD + 4}), ("ld_small", {"ld": 3 * HD - 8}),
               ("qkv_null", {"qkv": None}), ("ctx_null", {"ctx": None}), ("ldc_small", {"ldc": HD - 8}), ("ldc_unaligned", {"ldc": HD + 4})]
        if bwd:
            bad += [("lse_null", {"lse": None}), ("dctx_null", {"dctx": None}), ("dqkv_null", {"dqkv": None}),
                    ("lddc_small", {"lddc": HD - 8}), ("lddc_unaligned", {"lddc": HD + 4}),
                    ("lddq_small", {"lddq": 3 * HD - 8}), ("lddq_unaligned", {"lddq": 3 * HD + 4})]
        if "varlen" in name:
            bad += [("cu_null", {"cu_seqlens": None})]
        if bwd and tiled:
            bad += [("delta_ws_null", {"delta_ws": None})]
        if tiled:                                       # B * heads is the leading factor of the 1-D grid
            bad += [("grid_overflow", {"B": 1 << 30, "heads": 4, "Hd": 256, "ld": 768, "ldc": 256, "lddc": 256, "lddq": 768})]
        if drop:
            bad += [("p_one", {"p": 1.0}), ("p_negative", {"p": -0.1}), ("first_sequence_negative", {"first_sequence": -1})]
        for label, override in bad:
            args = [override[n] if n in override else VALID.get(n, PTR) for n in names]
            yield pytest.param(name, args, id=f"{name}-{label}")


@pytest.mark.parametrize("name,args", list(_cases()))
def test_attention_rejects_bad_arguments(name, args):
    lib = _hip.load()
    rc = getattr(lib, name)(*args)
    assert rc != 0
    message = lib.mmg_last_error().decode()
    assert message.startswith(name + ":"), message
    assert "launch failed" not in message, message          # rejected by validation, not by a launch that went wrong
