"""``MOTIONCLIP`` and ``get_SAG`` drop-ins (``scripts/model/motionclip.py``): the SAG model as one module, so that ``SAG.pth`` loads
the way the reference loads it (``encoder.*`` / ``decoder.*`` keys) and ``SAG(batch)``, ``SAG.encoder(batch)`` and
``SAG.decoder(batch)`` all exist.  Both halves run on the gfx950 engines (``motionclip_module``); there is no CPU path.

Inference only: ``compute_loss`` (the reconstruction / velocity / CLIP-cosine training objective) is not built.  ``get_SAG`` returns
``None`` where the reference returns the CLIP text encoder (it would have to fetch CLIP's weights); ``get_clip`` builds that encoder
from a CLIP state dict the caller already has (``clip_text.CLIPTextEncoder``), and ``motion_text_cosine`` scores a motion latent
against its features."""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib
from .clip_text import CLIPTextEncoder, load_clip_text
from .motionclip_module import Decoder_TRANSFORMER, Encoder_TRANSFORMER


def motion_text_cosine(z, text_features):
    """The ``cos`` of ``MOTIONCLIP.compute_clip_losses`` (motionclip.py:54-62): both sides are L2-normalised, then
    ``nn.CosineSimilarity(dim=1, eps=1e-6)``.  Plain torch on whatever device the tensors are on; returns [B]."""
    unit = [torch.as_tensor(t) for t in (text_features, z)]
    unit = [t / torch.linalg.vector_norm(t, dim=-1, keepdim=True) for t in unit]
    return nn.functional.cosine_similarity(unit[0], unit[1], dim=1, eps=1e-6)


class MOTIONCLIP(nn.Module):
    def __init__(self, encoder, decoder, promptLearner, cfg):
        super().__init__()
        self.encoder = encoder
        self.decoder = decoder
        self.promptLearner = promptLearner
        self.cfg = cfg

    def compute_loss(self, batch, clip_model):
        raise NotImplementedError("SAG training (compute_loss, motionclip_loss.py) is not built: this module runs inference only")

    @staticmethod
    def lengths_to_mask(lengths):
        """[n] clip lengths -> [n, max(lengths)] bool, True on the frames a clip has."""
        frames = torch.arange(int(lengths.max()), device=lengths.device)
        return frames[None, :] < lengths[:, None]

    def forward(self, batch, wait=True):
        """encode -> ``batch['z'] = batch['mu']`` -> decode -> ``batch['output_xyz'] = batch['output']``.  ``mu`` stays on the device:
        the encode is enqueued on the encoder's stream and the decoder's stream is ordered behind it, with no host round trip.
        ``wait=False`` (no counterpart in the reference) leaves the decode enqueued too, as ``Decoder_TRANSFORMER.forward`` does.
        Two consumers read ``mu`` and each is ordered behind the encode: the decoder's stream (the decode itself) and torch's current
        stream (``encode(wait=False)`` does that: the decoder's ``final_z = z.clone()`` and whatever the caller does with ``mu``)."""
        x = batch["x"]
        on_device = isinstance(x, torch.Tensor) and x.is_cuda
        batch.update(self.encoder(batch, wait=not on_device))
        batch["z"] = batch["mu"]
        if on_device:
            enc, dec = self.encoder.engine(), self.decoder.engine()
            _lib.stream_order(enc.device, enc._stream, dec._stream)
        batch.update(self.decoder(batch, wait=wait))
        batch["output_xyz"] = batch["output"]
        return batch


def get_SAG(cfg):
    """``(MOTIONCLIP, textEncoder)`` as the reference's ``get_SAG`` returns them, with ``textEncoder = None``: in the reference the
    second item is the CLIP ViT-B/32 text encoder, loaded from the network; ``get_clip`` builds it from a state dict instead.  ``cfg``
    needs ``n_pre_poses`` and ``use_style``."""
    halves = (Encoder_TRANSFORMER(latent_dim=512),          # encoder first: a seeded get_SAG draws its parameters before the decoder's
              Decoder_TRANSFORMER(latent_dim=512, n_pre_poses=cfg.n_pre_poses, use_style=cfg.use_style))
    return MOTIONCLIP(*halves, promptLearner=None, cfg=cfg), None


def get_clip(state_dict_or_path, device="cuda"):
    """The reference's ``get_clip()`` (motionclip.py:96-104) without its download: a ``CLIPTextEncoder`` loaded from a CLIP state dict
    the caller has -- a dict, or the path of a file ``torch.load`` / ``torch.jit.load`` reads (``clip_model.state_dict()`` saved, or the
    ViT-B/32 archive itself).  Nothing is ever fetched.  Sizes are read off the tensors; the image tower's keys are dropped
    (``load_clip_text``).  Returns the encoder on ``device``, frozen and in eval mode, as the reference leaves its CLIP."""
    sd = state_dict_or_path
    if not isinstance(sd, dict):
        try:
            sd = torch.jit.load(state_dict_or_path, map_location="cpu").state_dict()
        except RuntimeError:
            sd = torch.load(state_dict_or_path, map_location="cpu")
        if not isinstance(sd, dict):
            sd = sd.state_dict()
    layers = len({k.split(".")[2] for k in sd if k.startswith("transformer.resblocks.")})
    width = sd["ln_final.weight"].shape[0]
    model = CLIPTextEncoder(embed_dim=sd["text_projection"].shape[1], context_length=sd["positional_embedding"].shape[0],
                            vocab_size=sd["token_embedding.weight"].shape[0], transformer_width=width,
                            transformer_heads=width // 64, transformer_layers=layers)
    load_clip_text(model, sd)
    return model.to(device).eval()
