"""``CLIPTextEncoder``: the text tower of CLIP (``clip_model.encode_text``) as a module of this package, so that the SAG chain --
tokens -> text features -> ``Decoder_TRANSFORMER`` -> refinement -- needs no second model from the third-party ``clip`` package.
Callers keep ``clip.tokenize`` (host-side, pure Python, needs CLIP's vocabulary file) and swap ``clip_model.encode_text``.

The parameters sit under CLIP's own state-dict names, so a CLIP checkpoint's text half loads as it is (``load_clip_text``); they
are evaluated in fp32 by the gfx950 engine (``ls_clip_text_encode``), as the reference evaluates them (``.float()``).  There is no
CPU execution path: the torch parameters only hold the weights.

Only rows ``0 .. eot`` of every sentence are computed, packed back to back: the attention mask is causal and only the row at the
end-of-text token is read out, so the rows behind it cannot reach the result."""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib

# what a whole CLIP state dict holds beside the text tower: the image tower, the logit scale and the JIT archive's three constants
_FOREIGN = ("logit_scale", "input_resolution", "context_length", "vocab_size")


class _Holder(nn.Module):
    """Parameters under a CLIP name that is a bare module attribute there (``attn.in_proj_weight``, ``out_proj``, ...)."""


class CLIPTextEncoder(nn.Module):
    """Defaults are ViT-B/32's text tower.  ``encode_text(text)`` takes ``[B, context_length]`` integer token ids (what
    ``clip.tokenize`` returns) and returns fp32 features ``[B, embed_dim]``."""

    def __init__(self, embed_dim=512, context_length=77, vocab_size=49408, transformer_width=512, transformer_heads=8,
                 transformer_layers=12):
        super().__init__()
        self.embed_dim, self.context_length, self.vocab_size = embed_dim, context_length, vocab_size
        self.transformer_width, self.transformer_heads, self.transformer_layers = transformer_width, transformer_heads, transformer_layers
        W = transformer_width
        self.token_embedding = nn.Embedding(vocab_size, W)
        self.positional_embedding = nn.Parameter(torch.empty(context_length, W))
        self.transformer = _Holder()
        self.transformer.resblocks = nn.ModuleList()
        for _ in range(transformer_layers):
            blk = _Holder()
            blk.ln_1, blk.ln_2 = nn.LayerNorm(W), nn.LayerNorm(W)
            blk.attn = _Holder()
            blk.attn.in_proj_weight = nn.Parameter(torch.empty(3 * W, W))
            blk.attn.in_proj_bias = nn.Parameter(torch.zeros(3 * W))
            blk.attn.out_proj = nn.Linear(W, W)
            blk.mlp = _Holder()
            blk.mlp.c_fc, blk.mlp.c_proj = nn.Linear(W, 4 * W), nn.Linear(4 * W, W)
            self.transformer.resblocks.append(blk)
        self.ln_final = nn.LayerNorm(W)
        self.text_projection = nn.Parameter(torch.empty(W, embed_dim))
        self.initialize_parameters()
        self.requires_grad_(False)
        self._engine = None
        self._weights_dirty = True

    def initialize_parameters(self):
        """CLIP.initialize_parameters, the text half."""
        W, L = self.transformer_width, self.transformer_layers
        nn.init.normal_(self.token_embedding.weight, std=0.02)
        nn.init.normal_(self.positional_embedding, std=0.01)
        proj_std, attn_std, fc_std = (W ** -0.5) * ((2 * L) ** -0.5), W ** -0.5, (2 * W) ** -0.5
        for blk in self.transformer.resblocks:
            nn.init.normal_(blk.attn.in_proj_weight, std=attn_std)
            nn.init.normal_(blk.attn.out_proj.weight, std=proj_std)
            nn.init.normal_(blk.mlp.c_fc.weight, std=fc_std)
            nn.init.normal_(blk.mlp.c_proj.weight, std=proj_std)
        nn.init.normal_(self.text_projection, std=W ** -0.5)

    def load_state_dict(self, state_dict, strict=True, **kw):
        res = super().load_state_dict(state_dict, strict=strict, **kw)
        self._weights_dirty = True
        return res

    def _apply(self, fn, *a, **k):
        res = super()._apply(fn, *a, **k)
        self._weights_dirty = True
        return res

    def engine(self) -> "_lib.ClipTextEngine":
        dev = self.text_projection.device
        if dev.type == "cuda":
            di = dev.index if dev.index is not None else torch.cuda.current_device()
        elif torch.cuda.is_available():
            di = torch.cuda.current_device()
        else:
            raise _lib.EngineError("no MI355X visible: livelyspeaker_amd has no CPU path")
        if self._engine is None or self._engine.device != di:
            self._engine = _lib.ClipTextEngine(self.vocab_size, self.context_length, self.transformer_width, self.transformer_heads,
                                               self.transformer_layers, self.embed_dim, device=di)
            self._weights_dirty = True
        if self._weights_dirty:
            self._engine.load_state_dict({k: v.detach().float().cpu().numpy() for k, v in self.state_dict().items()})
            self._weights_dirty = False
        return self._engine

    def encode_text(self, text, wait=True, prune=True):
        """``text`` [B, context_length] integer ids -> features [B, embed_dim] fp32, on the tokens' device when they are a CUDA tensor
        and on the module's device otherwise.  Host tokens are planned on the host; device tokens cost one host wait (the packed row
        count comes back).  ``wait=False`` (no counterpart in CLIP): the encode stays enqueued on the encoder's stream; torch's current
        stream is ordered behind it, a consumer on another stream by ``_lib.stream_order(device, self.engine()._stream, that_stream)``.
        ``prune=False`` computes all rows of every sentence: the same bits, there to test and time the packing against."""
        if not isinstance(text, torch.Tensor):
            text = torch.as_tensor(text)
        if text.dtype.is_floating_point or text.dtype == torch.bool:
            raise TypeError(f"text holds token ids (an integer tensor), got {text.dtype}")
        if text.dim() != 2 or text.shape[1] != self.context_length:
            raise ValueError(f"text must be [B, {self.context_length}], got {list(text.shape)}")
        eng = self.engine()
        out = eng.encode(text.long(), wait=wait, prune=prune, device_out=True)
        dev = text.device if text.is_cuda else self.text_projection.device
        return out.to(dev)

    forward = encode_text


def load_clip_text(model: CLIPTextEncoder, state_dict) -> CLIPTextEncoder:
    """Load the text half of a whole CLIP state dict (``clip_model.state_dict()`` or the JIT archive's): ``visual.*``, ``logit_scale``
    and the archive's ``input_resolution`` / ``context_length`` / ``vocab_size`` are dropped, the rest is cast to fp32 (CLIP ships
    fp16) and must match the model's keys exactly -- any other unexpected key and any missing key raise, as ``load_model_wo_clip``
    does."""
    text = {k: v.float() if isinstance(v, torch.Tensor) else torch.as_tensor(v).float()
            for k, v in state_dict.items() if not (k.startswith("visual.") or k in _FOREIGN)}
    missing_keys, unexpected_keys = model.load_state_dict(text, strict=False)
    if unexpected_keys:
        raise KeyError(f"unexpected keys in the CLIP state dict: {sorted(unexpected_keys)}")
    if missing_keys:
        raise KeyError(f"keys missing from the CLIP state dict: {sorted(missing_keys)}")
    return model
