"""Writes the textual-inversion fixtures of tests/golden/ (embeddings.json, embeddings.npz) from the reference's own prompt path.

The reference is read where it lies (oracle.extract_ref): its SDTokenizer, SDClipModel and ClipTokenWeightEncoder are executed from its file, and
this tool executes two more of its definitions (expand_directory_list, load_embed) into the same namespace; none of its text is copied.
The embedding files are written into a temporary directory (tests/embedding_files.py, the writer the tests use too) from
weights.synth_tensor values at the scale of the token embeddings.  SDTokenizer(embedding_directory=tmp) runs on the reference checkout's full
tokenizer files; SDClipModel runs on the tiny CLIP configuration (written as a temporary JSON file) with weights.synth_state_dict.

Recorded per prompt: the chunk structure (a vector slot as ["e", file, row]), the ids after set_up_textual_embeddings (with the empty row of a
weighted prompt), the order of the custom vectors in the rebuilt table, cond, pooled, and the rel-L2 between cond and the reference's cond for
the same prompt with its `embedding:` words deleted (the shorter of two conds of unequal length is zero-padded: a prompt that loses a chunk
without its embedding).  That distance must be at least 10 x the end-to-end bound of tests/test_embeddings_gpu.py, or this tool fails.

    python tools/make_embedding_golden.py
"""
import ast
import json
import os
import sys
import tempfile
import traceback

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from lightdiffusion_amd import weights as W                    # noqa: E402
from embedding_files import write_embedding_files     # noqa: E402
from oracle.extract_ref import REF_PATH, load_reference        # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
E2E_BOUND = 5e-3          # tests/test_models_gpu.py::test_clip_text_model_on_hip_kernels: this text model against the reference
EXTRA_DEFS = ("expand_directory_list", "load_embed")
SHAPES = {"one": (64,), "three": (3, 64), "ten": (10, 64), "lst": (2, 64), "nested": (1, 64), "wide": (2, 96)}
FILLER = lambda n: " ".join(["cat"] * n)
PROMPTS = {
    "one_row_1d": "a photo of embedding:one cat",
    "three_rows": "a photo of embedding:three cat",
    "ten_rows": "embedding:ten a cat",
    "four_formats": "a embedding:ten cat embedding:three on embedding:lst grass embedding:nested",
    "comma_leftover": "a cat, embedding:three, on grass",
    "weighted": "a (embedding:three:1.3) cat",
    "missing_name": "a embedding:nothere cat embedding:one",
    "wrong_width_pad_quirk": "a embedding:wide cat embedding:three",
    "filler75_three_moves": FILLER(75) + " embedding:three",
    "filler75_ten": FILLER(75) + " embedding:ten",
    "filler70_ten_splits": FILLER(70) + " embedding:ten",
}


def rel_l2(a, b):
    n = max(a.shape[-2], b.shape[-2])
    pad = lambda t: torch.cat([t, t.new_zeros(*t.shape[:-2], n - t.shape[-2], t.shape[-1])], dim=-2)
    a, b = pad(a).double(), pad(b).double()
    return float((a - b).norm() / b.norm())


def main():
    torch.set_grad_enabled(False)
    os.environ.setdefault("HF_HUB_OFFLINE", "1")
    from transformers import CLIPTokenizer
    ref = load_reference()
    ns = ref.SDTokenizer.__init__.__globals__           # the namespace the reference's definitions were executed in
    ns.update(os=os, traceback=traceback)
    for node in ast.parse(open(REF_PATH).read(), REF_PATH).body:
        if getattr(node, "name", None) in EXTRA_DEFS:
            exec(compile(ast.Module([node], []), REF_PATH, "exec"), ns)
    assert all(n in ns for n in EXTRA_DEFS)

    cfg = W.tiny_clip_config()
    V, h = cfg["vocab_size"], cfg["hidden_size"]
    vectors = {n: W.synth_tensor(f"embeddings.{n}.token_embedding.weight", s) for n, s in SHAPES.items()}
    with tempfile.TemporaryDirectory() as tmp:
        emb_dir = write_embedding_files(os.path.join(tmp, "embeddings"), vectors)
        for n, v in vectors.items():                    # what the reference's loader makes of every file
            got = ns["load_embed"](n, emb_dir, h, "clip_l")
            assert got.shape == v.shape and torch.equal(got, v), n
        with open(os.path.join(tmp, "clip.json"), "w") as f:
            json.dump(cfg, f)
        tok = ref.SDTokenizer(tokenizer_path=os.path.join(os.path.dirname(REF_PATH), "_internal", "sd1_tokenizer"), tokenizer_class=CLIPTokenizer,
                              embedding_directory=emb_dir, embedding_size=h)
        plain = ref.SDTokenizer(tokenizer_path=os.path.join(os.path.dirname(REF_PATH), "_internal", "sd1_tokenizer"), tokenizer_class=CLIPTokenizer)
        word_ids, inner = {}, tok.tokenizer

        def recording(word):
            r = inner(word)
            word_ids[word] = r["input_ids"][1:-1]
            return r
        tok.tokenizer = recording

        clip = ref.SDClipModel(device="cpu", dtype=torch.float32, textmodel_json_config=os.path.join(tmp, "clip.json"))
        sd = W.synth_state_dict(W.clip_param_shapes(cfg))
        missing = clip.transformer.load_state_dict(sd, strict=False)
        assert list(missing.missing_keys) == ["text_projection.weight"] and not missing.unexpected_keys, missing
        seen = {}
        set_up, set_emb = clip.set_up_textual_embeddings, clip.transformer.set_input_embeddings

        def rec_set_up(tokens, current):
            seen["ids"] = set_up(tokens, current)
            return seen["ids"]

        def rec_set_emb(e):
            if e.weight.shape[0] > V and "table" not in seen:
                seen["table"] = e.weight[V - 1:-1].clone()
            set_emb(e)
        clip.set_up_textual_embeddings, clip.transformer.set_input_embeddings = rec_set_up, rec_set_emb

        def slot(t):
            if not isinstance(t, torch.Tensor):
                return int(t)
            for n, v in vectors.items():
                for r, row in enumerate(v.reshape(-1, v.shape[-1])):
                    if row.shape == t.shape and torch.equal(row, t):
                        return ["e", n, r]
            raise AssertionError("a vector no file holds")

        out, arrays = {}, {f"vec_{n}": v.numpy() for n, v in vectors.items()}
        for key, prompt in PROMPTS.items():
            chunks = tok.tokenize_with_weights(prompt)
            seen.clear()
            cond, pooled = clip.encode_token_weights(chunks)
            ids, table = seen["ids"], seen.get("table", torch.zeros(0, h))
            deleted = " ".join(w for w in prompt.split(" ") if "embedding:" not in w)
            cond_del, _ = clip.encode_token_weights(plain.tokenize_with_weights(deleted))
            dist = rel_l2(cond_del, cond)
            out[key] = {"prompt": prompt, "chunks": [[[slot(t), float(w)] for t, w in c] for c in chunks], "ids": ids,
                        "side_table": [slot(r) for r in table], "deleted_prompt": deleted, "deleted_rel_l2": dist}
            arrays[f"cond_{key}"], arrays[f"pooled_{key}"] = cond.numpy(), pooled.numpy()
            print(f"{key}: {len(chunks)} chunk(s), E = {table.shape[0]}, cond {tuple(cond.shape)}, distance without the embedding words {dist:.3f}")
            assert dist >= 10 * E2E_BOUND, f"{key}: the embedding moves cond by only {dist:.3e}: choose other vectors or another prompt"
    with open(os.path.join(GOLDEN, "embeddings.json"), "w") as f:
        json.dump({"config": cfg, "files": {n: list(s) for n, s in SHAPES.items()}, "word_ids": word_ids, "prompts": out}, f)
    np.savez_compressed(os.path.join(GOLDEN, "embeddings.npz"), **arrays)
    print("wrote embeddings.json, embeddings.npz;", len(word_ids), "words")


if __name__ == "__main__":
    main()
