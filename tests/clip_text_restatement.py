"""The CLIP text tower restated in numpy float64 (not a test module), in the two forms the engine has, and the torch module the tests
hold both against.

``ClipTextRestatement.encode(tokens, prune=True)`` runs every sentence at its own length ``eot + 1`` -- what the packed rows of the
HIP path compute; ``prune=False`` runs all 77 rows under the causal mask, as CLIP does.  ``TorchClipText`` is CLIP's ``encode_text``
assembled from ``nn.MultiheadAttention``, ``nn.LayerNorm`` and ``nn.Linear`` in a chosen dtype: in float64 it is the yardstick of the
restatement, in float32 on the CPU it measures the rounding the fp32 arithmetic itself has (the GPU tests' unit of error)."""
import functools

import numpy as np
import torch
import torch.nn as nn

from livelyspeaker_amd import synth

HEADS = 8
LENGTHS = [2, 15, 16, 17, 33, 77, 5]        # the minimal sentence, both sides of a 16-row tile edge, two tiles + 1, the full context, ragged
LENGTHS_12 = [2, 17, 77, 5]                 # the 12-layer cases: four of them


@functools.lru_cache(maxsize=None)
def state(layers):
    return synth.synth_clip_text_state(layers=layers)


def layer_norm(x, w, b):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + 1e-5) * w + b


class ClipTextRestatement:
    def __init__(self, sd, heads=HEADS):
        self.emb = sd["token_embedding.weight"]          # gathered rows are widened; the table stays as it is
        self.w = {k: np.asarray(v, np.float64) for k, v in sd.items() if k != "token_embedding.weight"}
        self.heads = heads
        self.layers = len({k.split(".")[2] for k in sd if k.startswith("transformer.resblocks.")})

    def _tower(self, x):
        """x [S, W]: one sentence's rows under the causal mask -> [S, W] after ln_final"""
        w, H = self.w, self.heads
        S, W = x.shape
        hd = W // H
        mask = np.triu(np.full((S, S), -np.inf), 1)
        for i in range(self.layers):
            p = f"transformer.resblocks.{i}."
            y = layer_norm(x, w[p + "ln_1.weight"], w[p + "ln_1.bias"])
            qkv = y @ w[p + "attn.in_proj_weight"].T + w[p + "attn.in_proj_bias"]
            q, k, v = (qkv[:, j * W:(j + 1) * W].reshape(S, H, hd).transpose(1, 0, 2) for j in range(3))
            s = (q * hd ** -0.5) @ k.transpose(0, 2, 1) + mask
            e = np.exp(s - s.max(-1, keepdims=True))
            a = (e / e.sum(-1, keepdims=True)) @ v
            x = x + a.transpose(1, 0, 2).reshape(S, W) @ w[p + "attn.out_proj.weight"].T + w[p + "attn.out_proj.bias"]
            h = layer_norm(x, w[p + "ln_2.weight"], w[p + "ln_2.bias"]) @ w[p + "mlp.c_fc.weight"].T + w[p + "mlp.c_fc.bias"]
            h = h / (1.0 + np.exp(-1.702 * h))
            x = x + h @ w[p + "mlp.c_proj.weight"].T + w[p + "mlp.c_proj.bias"]
        return layer_norm(x, w["ln_final.weight"], w["ln_final.bias"])

    def encode(self, tokens, prune=True):
        tokens = np.asarray(tokens)
        out = np.empty((tokens.shape[0], self.w["text_projection"].shape[1]))
        for b, row in enumerate(tokens):
            eot = int(np.argmax(row))                    # numpy's argmax is the first position of the maximum, like torch's
            n = eot + 1 if prune else len(row)
            x = self.emb[row[:n]].astype(np.float64) + self.w["positional_embedding"][:n]
            out[b] = self._tower(x)[eot] @ self.w["text_projection"]
        return out


class TorchClipText(nn.Module):
    """CLIP.encode_text from torch's own layers, evaluated in ``dtype`` on the CPU (or wherever it is moved)."""

    def __init__(self, sd, dtype=torch.float64, heads=HEADS):
        super().__init__()
        t = lambda k: torch.as_tensor(sd[k]).to(dtype)
        W = sd["ln_final.weight"].shape[0]
        self.layers = len({k.split(".")[2] for k in sd if k.startswith("transformer.resblocks.")})
        self.register_buffer("emb", torch.as_tensor(sd["token_embedding.weight"]))     # fp32 table; rows are cast after the gather (exact)
        self.register_buffer("pos", t("positional_embedding"))
        self.register_buffer("proj", t("text_projection"))
        self.blocks = nn.ModuleList()
        for i in range(self.layers):
            p = f"transformer.resblocks.{i}."
            blk = nn.ModuleDict({"ln_1": nn.LayerNorm(W), "attn": nn.MultiheadAttention(W, heads), "ln_2": nn.LayerNorm(W),
                                 "c_fc": nn.Linear(W, 4 * W), "c_proj": nn.Linear(4 * W, W)}).to(dtype)
            own = {"ln_1.weight": blk["ln_1"].weight, "ln_1.bias": blk["ln_1"].bias, "ln_2.weight": blk["ln_2"].weight,
                   "ln_2.bias": blk["ln_2"].bias, "attn.in_proj_weight": blk["attn"].in_proj_weight,
                   "attn.in_proj_bias": blk["attn"].in_proj_bias, "attn.out_proj.weight": blk["attn"].out_proj.weight,
                   "attn.out_proj.bias": blk["attn"].out_proj.bias, "mlp.c_fc.weight": blk["c_fc"].weight, "mlp.c_fc.bias": blk["c_fc"].bias,
                   "mlp.c_proj.weight": blk["c_proj"].weight, "mlp.c_proj.bias": blk["c_proj"].bias}
            with torch.no_grad():
                for k, dst in own.items():
                    dst.copy_(t(p + k))
            self.blocks.append(blk)
        self.ln_final = nn.LayerNorm(W).to(dtype)
        with torch.no_grad():
            self.ln_final.weight.copy_(t("ln_final.weight"))
            self.ln_final.bias.copy_(t("ln_final.bias"))
        self.requires_grad_(False).eval()

    @torch.no_grad()
    def forward(self, text):
        text = torch.as_tensor(text).to(self.pos.device)
        S = text.shape[1]
        x = self.emb[text].to(self.pos.dtype) + self.pos[:S]
        x = x.permute(1, 0, 2)                           # NLD -> LND
        mask = torch.full((S, S), float("-inf"), dtype=x.dtype, device=x.device).triu_(1)
        for blk in self.blocks:
            y = blk["ln_1"](x)
            x = x + blk["attn"](y, y, y, need_weights=False, attn_mask=mask)[0]
            h = blk["c_fc"](blk["ln_2"](x))
            x = x + blk["c_proj"](h * torch.sigmoid(1.702 * h))
        x = self.ln_final(x.permute(1, 0, 2))
        return x[torch.arange(x.shape[0], device=x.device), text.argmax(dim=-1)] @ self.proj
