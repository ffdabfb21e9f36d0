"""CPU reference of the ViT tower under patch dropout: the arithmetic of oracle.encoders_oracle.vit_forward, written anew in torch fp32, with
the kept patches selected after the position add - x = cat(x[:, :1], x[:, 1:][b, keep[b]]) - as FLIP and open_clip do.  `keep` comes from
mmgclip.patch_dropout.keep_indices, the numpy statement of the draw, which is re-exported here.  With the identity keep it IS vit_forward
(tests/test_patch_dropout_cpu.py holds it to that by torch.equal).  Same role as tests/augment_ref.py."""
import torch
import torch.nn.functional as F

from mmgclip.patch_dropout import keep_count, keep_indices  # noqa: F401  (what the tests draw with)


def vit_forward_kept(sd, images, keep, heads=12, patch=16, scale16=True, prefix=""):
    """sd: torchvision vit_b_16-layout state dict (fp32); images fp32 [n, Cin, H, W] in [0, 1]; keep: int [n, K] (array or tensor), the patches
    every image keeps, ascending.  -> the class token after encoder.ln, [n, hidden]."""
    g = lambda k: sd[prefix + k]                                           # noqa: E731
    x = images
    if scale16:
        x = (65535.0 * x - 32767.5) / 32767.5
    x = F.conv2d(x, g("conv_proj.weight"), g("conv_proj.bias"), stride=patch)
    B, H = x.shape[0], x.shape[1]
    x = x.flatten(2).transpose(1, 2)
    x = torch.cat([g("class_token").expand(B, -1, -1), x], dim=1) + g("encoder.pos_embedding")
    keep = torch.as_tensor(keep).to(torch.int64)
    assert keep.shape[0] == B and keep.dim() == 2
    rows = torch.arange(B)[:, None]
    x = torch.cat([x[:, :1], x[:, 1:][rows, keep]], dim=1)
    S = x.shape[1]
    i = 0
    while prefix + f"encoder.layers.encoder_layer_{i}.ln_1.weight" in sd:
        p = f"encoder.layers.encoder_layer_{i}."
        y = F.layer_norm(x, (H,), g(p + "ln_1.weight"), g(p + "ln_1.bias"), 1e-6)
        qkv = F.linear(y, g(p + "self_attention.in_proj_weight"), g(p + "self_attention.in_proj_bias"))
        q, k, v = (t.view(B, S, heads, H // heads).permute(0, 2, 1, 3) for t in qkv.chunk(3, dim=-1))
        a = ((q @ k.transpose(-1, -2)) / (H // heads) ** 0.5).softmax(-1) @ v
        a = a.permute(0, 2, 1, 3).reshape(B, S, H)
        x = x + F.linear(a, g(p + "self_attention.out_proj.weight"), g(p + "self_attention.out_proj.bias"))
        z = F.layer_norm(x, (H,), g(p + "ln_2.weight"), g(p + "ln_2.bias"), 1e-6)
        x = x + F.linear(F.gelu(F.linear(z, g(p + "mlp.0.weight"), g(p + "mlp.0.bias"))), g(p + "mlp.3.weight"), g(p + "mlp.3.bias"))
        i += 1
    x = F.layer_norm(x, (H,), g("encoder.ln.weight"), g("encoder.ln.bias"), 1e-6)
    return x[:, 0]
