"""Textual-inversion files for the embedding tests and for tools/make_embedding_golden.py: one directory with every on-disk layout the
loader reads, written from the vectors of tests/golden/embeddings.npz (so the generator's reference run and the tests see the same files).
Not a test module."""
import os

import torch

# name -> (path under the directory, layout); the vectors of `name` are what a correct load returns
LAYOUTS = {
    "one": ("one.pt", "first_value"),              # a 1-D vector, under a key of no special meaning
    "three": ("three.safetensors", "clip_l"),      # 'clip_l' beside a 'clip_g' decoy that sorts first
    "ten": ("ten.pt", "string_to_param"),          # the A1111 layout
    "lst": ("lst.bin", "list_of_dicts"),           # a list of dicts; tensors of another width are skipped
    "nested": (os.path.join("sub", "deeper", "nested.pt"), "clip_l"),
    "wide": ("wide.safetensors", "clip_l"),        # rows wider than the text model: refused where they are used
}


def write_embedding_files(root, vectors):
    """vectors: {name: fp32 tensor}.  Returns root."""
    import safetensors.torch
    for name, (rel, layout) in LAYOUTS.items():
        v = vectors[name].clone().contiguous()
        path = os.path.join(root, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        decoy = torch.full((max(v.shape[0], 1) if v.dim() > 1 else 1, v.shape[-1] // 2), 7.0)
        if layout == "first_value":
            obj = {"emb_params": v}
        elif layout == "string_to_param":
            obj = {"string_to_name": {"*": 265}, "string_to_param": {"*": v}, "name": name, "step": 1000}
        elif layout == "list_of_dicts":
            obj = [{"clip_g": decoy, "clip_l": v[:1]}, {"clip_l": v[1:]}]
        else:
            obj = {"clip_g": decoy, "clip_l": v}
        if rel.endswith(".safetensors"):
            safetensors.torch.save_file(obj, path)
        else:
            torch.save(obj, path)
    return root
