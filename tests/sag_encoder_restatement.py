"""CPU restatement (numpy float64) of the SAG encoder, Encoder_TRANSFORMER.forward in eval mode (scripts/model/motionclip_module.py:
70-95), and of the motion-to-text cosine (scripts/model/motionclip.py:54-62).  Not a test module.  Pinned to the reference by
tests/test_sag_encoder.py (fixture G19) before anything on the GPU is compared with it.

``pruned=True`` states the last layer the way the HIP path runs it: K and V for all 36 tokens, everything else for token 0 alone.
It is the same function (only token 0 leaves the encoder); both forms are kept so that the tests pin their agreement."""
import math

import numpy as np

F64 = np.float64
_erf = np.vectorize(math.erf, otypes=[F64])


def positional_encoding(rows, d):
    """PositionalEncoding.pe[:rows] as the fp32 torch buffer holds it (motionclip_module.py:12-24)."""
    pos = np.arange(rows, dtype=np.float32)[:, None]
    div = np.exp(np.arange(0, d, 2, dtype=np.float32) * np.float32(-math.log(10000.0) / d)).astype(np.float32)
    pe = np.zeros((rows, d), np.float32)
    pe[:, 0::2] = np.sin(pos * div)
    pe[:, 1::2] = np.cos(pos * div)
    return pe


def _layernorm(x, w, b):
    mean = x.mean(-1, keepdims=True)
    var = ((x - mean) ** 2).mean(-1, keepdims=True)
    return (x - mean) / np.sqrt(var + 1e-5) * w + b


def _gelu(x):
    return 0.5 * x * (1.0 + _erf(x / math.sqrt(2.0)))


class SagEncoderRestatement:
    def __init__(self, sd, njoints=9, nfeats=3, num_layers=3, num_heads=4):
        self.sd = {k: np.asarray(v, dtype=F64) for k, v in sd.items() if not k.endswith(".pe")}
        self.jf, self.L, self.H = njoints * nfeats, num_layers, num_heads

    def _attention(self, q, k, v, keep):
        """q [B, Sq, D], k / v [B, S, D], keep [B, S] bool -> [B, Sq, D]; a padded key scores -inf, so its probability is exactly 0."""
        B, Sq, D = q.shape
        hd = D // self.H
        split = lambda a: a.reshape(B, a.shape[1], self.H, hd).transpose(0, 2, 1, 3)
        s = (split(q) / math.sqrt(hd)) @ split(k).transpose(0, 1, 3, 2)
        s = np.where(keep[:, None, None, :], s, -np.inf)
        p = np.exp(s - s.max(-1, keepdims=True))
        p /= p.sum(-1, keepdims=True)
        return (p @ split(v)).transpose(0, 2, 1, 3).reshape(B, Sq, D)

    def _layer(self, l, x, keep, rows):
        """Post-norm nn.TransformerEncoderLayer; `rows` selects the query tokens that are carried on (None = all)."""
        g = lambda n: self.sd[f"seqTransEncoder.layers.{l}.{n}"]
        D = x.shape[-1]
        wi, bi = g("self_attn.in_proj_weight"), g("self_attn.in_proj_bias")
        xq = x if rows is None else x[:, rows]
        q = xq @ wi[:D].T + bi[:D]
        k = x @ wi[D:2 * D].T + bi[D:2 * D]
        v = x @ wi[2 * D:].T + bi[2 * D:]
        a = self._attention(q, k, v, keep) @ g("self_attn.out_proj.weight").T + g("self_attn.out_proj.bias")
        y = _layernorm(xq + a, g("norm1.weight"), g("norm1.bias"))
        f = _gelu(y @ g("linear1.weight").T + g("linear1.bias")) @ g("linear2.weight").T + g("linear2.bias")
        return _layernorm(y + f, g("norm2.weight"), g("norm2.bias"))

    def encode(self, x, mask=None, pruned=False):
        """x [B, J, F, T], mask [B, T] bool or None -> mu [B, D] (float64)."""
        x = np.asarray(x, dtype=F64)
        B, T = x.shape[0], x.shape[-1]
        frames = x.reshape(B, self.jf, T).transpose(0, 2, 1)                               # [B, T, J*F]
        emb = frames @ self.sd["skelEmbedding.weight"].T + self.sd["skelEmbedding.bias"]
        D = emb.shape[-1]
        tok = np.concatenate([np.broadcast_to(self.sd["muQuery"].reshape(1, 1, D), (B, 1, D)),
                              np.broadcast_to(self.sd["sigmaQuery"].reshape(1, 1, D), (B, 1, D)), emb], axis=1)
        tok = tok + positional_encoding(T + 2, D).astype(F64)[None]
        keep = np.ones((B, T + 2), dtype=bool)
        if mask is not None:
            keep[:, 2:] = np.asarray(mask, dtype=bool)
        for l in range(self.L):
            tok = self._layer(l, tok, keep, [0] if pruned and l == self.L - 1 else None)
        return tok[:, 0]


def motion_text_cosine(z, text_features, eps=1e-6):
    """cos of compute_clip_losses: normalise both, then CosineSimilarity(dim=1, eps)."""
    z, t = np.asarray(z, dtype=F64), np.asarray(text_features, dtype=F64)
    zn, tn = z / np.linalg.norm(z, axis=-1, keepdims=True), t / np.linalg.norm(t, axis=-1, keepdims=True)
    return (zn * tn).sum(1) / (np.maximum(np.linalg.norm(zn, axis=1), eps) * np.maximum(np.linalg.norm(tn, axis=1), eps))
