"""Prompt encoding helpers with the call surface of the reference's ``orv/models/text_encoder.py`` (``compute_prompt_embeddings`` /
``encode_prompt`` / ``_get_t5_prompt_embeds``; the encoder call is its line 34, ``text_encoder(ids)[0]``, which the pipeline reaches at
``orv/models/cogvideox_control.py:1290-1299``).  ``text_encoder`` is ``orv_amd.t5.T5EncoderModel`` or any object with that call; the
tokenizer is delegated: transformers' ``T5Tokenizer`` or any callable of its call shape, or none at all when the caller already holds
token ids (``text_input_ids=``).  ``orv_amd.install()`` does not alias this module."""
from __future__ import annotations

import contextlib
from typing import List, Optional, Union

import torch


def _get_t5_prompt_embeds(tokenizer, text_encoder, prompt: Union[str, List[str]], num_videos_per_prompt: int = 1,
                          max_sequence_length: int = 226, device: Optional[torch.device] = None, dtype: Optional[torch.dtype] = None,
                          text_input_ids: Optional[torch.Tensor] = None) -> torch.Tensor:
    if tokenizer is not None:
        prompts = [prompt] if isinstance(prompt, str) else list(prompt)
        tokens = tokenizer(prompts, padding="max_length", max_length=max_sequence_length, truncation=True, add_special_tokens=True,
                           return_tensors="pt")
        text_input_ids = tokens.input_ids if hasattr(tokens, "input_ids") else tokens["input_ids"]
    elif text_input_ids is None:
        raise ValueError("without a tokenizer the token ids have to come from the caller: pass text_input_ids=")
    where = device if device is not None else getattr(text_encoder, "device", None)
    embeds = text_encoder(text_input_ids.to(where))[0].to(dtype=dtype, device=device)
    batch, seq_len, _ = embeds.shape                         # by the ids: without a tokenizer `prompt` may be None
    return embeds.repeat(1, num_videos_per_prompt, 1).view(batch * num_videos_per_prompt, seq_len, -1)


def encode_prompt(tokenizer, text_encoder, prompt: Union[str, List[str]], num_videos_per_prompt: int = 1, max_sequence_length: int = 226,
                  device: Optional[torch.device] = None, dtype: Optional[torch.dtype] = None,
                  text_input_ids: Optional[torch.Tensor] = None) -> torch.Tensor:
    return _get_t5_prompt_embeds(tokenizer, text_encoder, prompt, num_videos_per_prompt=num_videos_per_prompt,
                                 max_sequence_length=max_sequence_length, device=device, dtype=dtype, text_input_ids=text_input_ids)


def compute_prompt_embeddings(tokenizer, text_encoder, prompt, max_sequence_length: int, device: torch.device, dtype: torch.dtype,
                              requires_grad: bool = False, text_input_ids: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``requires_grad=False`` runs the call under ``torch.no_grad()``; ``True`` leaves the caller's grad mode as it is, as in the
    reference.  The native encoder is inference-only and never records a graph either way."""
    with contextlib.nullcontext() if requires_grad else torch.no_grad():
        return encode_prompt(tokenizer, text_encoder, prompt, num_videos_per_prompt=1, max_sequence_length=max_sequence_length,
                             device=device, dtype=dtype, text_input_ids=text_input_ids)
