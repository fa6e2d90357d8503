"""The motion latent: what stages A-D (shape encoder, image encoder, trunk) leave for the decoder.

``Motion_Latent_Model.encode_motion(sample)`` returns one, ``decode_motion(latent, points...)`` moves any point set by it;
``inference.run_model_inference(..., return_latent=True)`` returns a whole video's.  64 tokens of width 768 per frame in the
product configuration: fp32 [T, 64, 768] is 6 MB for 32 frames, against 88 % of the clip's FLOPs to compute it.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch

_FORMAT = 1


class MotionLatent:
    """tokens fp32 [B, T, K, C]: rows 4..4+K of every frame of the trunk's output stream (the rows the decoder reads), always
    the holder's own memory.  from_ref: frames of a long video that the driver's merge rules replace with ``ref_pcd`` whatever
    their tokens say (empty for a single clip).  d, K, frames: the encoding model's transformer.d, model.tokens and
    training.frames -- decode_motion refuses a latent whose d / K are not the decoding model's."""

    def __init__(self, tokens: torch.Tensor, d: int, K: int, frames: int, from_ref: Optional[Sequence[int]] = None):
        if tokens.dim() != 4 or tokens.shape[2] != K or tokens.shape[3] != d:
            raise ValueError(f"MotionLatent: tokens must be [B, T, {K}, {d}], got {tuple(tokens.shape)}")
        self.tokens = tokens.detach().to(torch.float32).contiguous()
        self.d, self.K, self.frames = int(d), int(K), int(frames)
        self.from_ref: List[int] = [int(t) for t in (from_ref or [])]

    def __repr__(self) -> str:
        return (f"MotionLatent(tokens={tuple(self.tokens.shape)} on {self.tokens.device}, d={self.d}, K={self.K}, "
                f"frames={self.frames}, from_ref={self.from_ref})")

    def to(self, device) -> "MotionLatent":
        return MotionLatent(self.tokens.to(device), self.d, self.K, self.frames, self.from_ref)

    def save(self, path: str) -> None:
        """A plain dict of tensors and ints: read back with ``torch.load(..., weights_only=True)`` like a checkpoint."""
        torch.save({"format": _FORMAT, "tokens": self.tokens.cpu(), "from_ref": torch.tensor(self.from_ref, dtype=torch.long),
                    "d": self.d, "K": self.K, "frames": self.frames}, path)

    @classmethod
    def load(cls, path: str, device="cpu") -> "MotionLatent":
        blob = torch.load(path, map_location=device, weights_only=True)
        if not isinstance(blob, dict) or blob.get("format") != _FORMAT or "tokens" not in blob:
            raise ValueError(f"{path}: not a MotionLatent file")
        return cls(blob["tokens"], blob["d"], blob["K"], blob["frames"], blob["from_ref"].tolist())
