"""Textual-inversion embedding files (`embedding:name` in a prompt): host-side lookup and parsing.

Mirrors: expand_directory_list / load_embed (LD.py:4795-4874).  The vectors a file yields go into the prompt's token groups
(`clip.PromptTokenizer`) and from there into the side table the input-stage kernel reads (`ops.clip_embed`).
"""
from __future__ import annotations

import logging
import os
import traceback
from typing import List, Optional, Sequence, Union

import torch

EXTENSIONS = (".safetensors", ".pt", ".bin")


def expand_directory_list(directories: Sequence[str]) -> List[str]:
    """every directory and all its sub-directories (links followed), each once, in walk order"""
    out: List[str] = []
    for d in directories:
        for root in [d] + [r for r, _, _ in os.walk(d, followlinks=True)]:
            if root not in out:
                out.append(root)
    return out


def find_embed_file(name: str, directories: Union[str, Sequence[str]]) -> Optional[str]:
    """The file `name` selects: in the first directory that has one, the exact name, else name + .safetensors / .pt / .bin in that order.
    A candidate that leaves its directory ('..', an absolute name) is skipped."""
    if isinstance(directories, (str, os.PathLike)):
        directories = [os.fspath(directories)]
    for d in expand_directory_list([os.fspath(x) for x in directories]):
        path, d = os.path.abspath(os.path.join(d, name)), os.path.abspath(d)
        try:
            if os.path.commonpath((d, path)) != d:
                continue
        except ValueError:
            continue
        if os.path.isfile(path):
            return path
        for ext in EXTENSIONS:
            if os.path.isfile(path + ext):
                return path + ext
    return None


def load_embed(name: str, directories: Union[str, Sequence[str]], embedding_size: int, embed_key: Optional[str] = "clip_l") -> Optional[torch.Tensor]:
    """The vectors of embedding `name`: fp32 [k, embedding_size] or [embedding_size] (as stored: a width that does not fit the text model is
    refused where the vectors are used), or None when no file is found or the file does not load (a warning, never an exception).
    .safetensors through safetensors, anything else through torch.load(weights_only=True): a pickle that needs more than tensors is not run."""
    path = find_embed_file(name, directories)
    if path is None:
        return None
    try:
        if path.lower().endswith(".safetensors"):
            import safetensors.torch
            embed = safetensors.torch.load_file(path, device="cpu")
        else:
            embed = torch.load(path, weights_only=True, map_location="cpu")
        if isinstance(embed, dict) and "string_to_param" in embed:              # the A1111 .pt layout
            out = next(iter(embed["string_to_param"].values()))
        elif isinstance(embed, list):
            rows = [t.reshape(-1, t.shape[-1]) for d in embed for t in d.values() if t.shape[-1] == embedding_size]
            out = torch.cat(rows, dim=0)
        elif embed_key is not None and embed_key in embed:
            out = embed[embed_key]
        else:
            out = next(iter(embed.values()))
        return out.detach().to(torch.float32)
    except Exception:
        logging.warning("%s\n\nerror loading embedding, skipping loading: %s", traceback.format_exc(), name)
        return None
