"""CPU: textual-inversion embeddings on the host — the file loader, `embedding:name` in the tokenizer, and the id remap / side table of
CLIP.encode_from_tokens, against what the reference's SDTokenizer and SDClipModel recorded (tools/make_embedding_golden.py)."""
import json
import logging
import os
import zlib

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from embedding_files import LAYOUTS, write_embedding_files


@pytest.fixture(scope="module")
def gold():
    g = json.load(open(os.path.join(GOLDEN, "embeddings.json")))
    with np.load(os.path.join(GOLDEN, "embeddings.npz")) as z:
        g["vectors"] = {n: torch.from_numpy(z["vec_" + n]) for n in g["files"]}
    return g


@pytest.fixture(scope="module")
def emb_dir(gold, tmp_path_factory):
    return write_embedding_files(str(tmp_path_factory.mktemp("embeddings")), gold["vectors"])


def slot(gold, t):
    """an id as it is; a vector as ["e", file, row], by its values"""
    if not isinstance(t, torch.Tensor):
        return t
    for n, v in gold["vectors"].items():
        for r, row in enumerate(v.reshape(-1, v.shape[-1])):
            if row.shape == t.shape and torch.equal(row, t):
                return ["e", n, r]
    raise AssertionError("a vector no file holds")


def tokenizer(gold, emb_dir):
    from lightdiffusion_amd.clip import PromptTokenizer
    return PromptTokenizer(lambda w: gold["word_ids"][w], embedding_directory=emb_dir, embedding_size=gold["config"]["hidden_size"])


# ------------------------------------------------------------------ load_embed
def test_load_embed_reads_every_layout(gold, emb_dir):
    from lightdiffusion_amd.embeddings import load_embed
    h = gold["config"]["hidden_size"]
    for name in LAYOUTS:
        got = load_embed(name, emb_dir, h)
        want = gold["vectors"][name]
        assert got.dtype == torch.float32 and got.shape == want.shape and torch.equal(got, want), name
    assert load_embed("one", emb_dir, h).dim() == 1
    assert torch.equal(load_embed("nested", [str(emb_dir)], h), gold["vectors"]["nested"])          # a list of directories; two levels down
    assert torch.equal(load_embed("nested", ["/nonexistent-dir", os.path.join(emb_dir, "sub")], h), gold["vectors"]["nested"])
    assert load_embed("nothere", emb_dir, h) is None
    # without the key the first value is taken: the 'clip_g' decoy of three.safetensors
    assert load_embed("three", emb_dir, h, embed_key=None).shape[-1] == h // 2
    # fp16 on disk comes back as fp32
    torch.save({"clip_l": gold["vectors"]["three"].half()}, os.path.join(emb_dir, "halfprec.pt"))
    got = load_embed("halfprec", emb_dir, h)
    assert got.dtype == torch.float32 and torch.equal(got, gold["vectors"]["three"].half().float())


def test_load_embed_extension_order_and_exact_name(tmp_path):
    import safetensors.torch
    from lightdiffusion_amd.embeddings import load_embed
    val = lambda x: torch.full((2, 8), float(x))
    torch.save({"clip_l": val(0)}, tmp_path / "x")                     # the exact name, no extension
    safetensors.torch.save_file({"clip_l": val(1)}, str(tmp_path / "x.safetensors"))
    torch.save({"clip_l": val(2)}, tmp_path / "x.pt")
    torch.save({"clip_l": val(3)}, tmp_path / "x.bin")
    assert float(load_embed("x.bin", str(tmp_path), 8)[0, 0]) == 3.0   # an exact file name wins over the extension search
    for want, gone in ((0.0, "x"), (1.0, "x.safetensors"), (2.0, "x.pt"), (3.0, "x.bin")):
        assert float(load_embed("x", str(tmp_path), 8)[0, 0]) == want
        os.remove(tmp_path / gone)
    assert load_embed("x", str(tmp_path), 8) is None


def test_load_embed_refuses_a_path_that_leaves_its_directory(tmp_path):
    from lightdiffusion_amd.embeddings import load_embed
    inside = tmp_path / "embeddings"
    inside.mkdir()
    torch.save({"clip_l": torch.ones(2, 8)}, tmp_path / "outside.pt")
    torch.save({"clip_l": torch.ones(2, 8)}, inside / "ok.pt")
    assert load_embed("ok", str(inside), 8) is not None
    assert load_embed("../outside", str(inside), 8) is None
    assert load_embed("../outside.pt", str(inside), 8) is None
    assert load_embed(str(tmp_path / "outside.pt"), str(inside), 8) is None
    assert load_embed(str(tmp_path / "outside"), str(inside), 8) is None


class _NeedsUnpickling:
    """a pickle that only torch.load(weights_only=False) would run: its __reduce__ makes a directory"""

    def __init__(self, marker):
        self.marker = marker

    def __reduce__(self):
        return (os.mkdir, (self.marker,))


def test_load_embed_bad_files_warn_and_give_none(tmp_path, caplog):
    from lightdiffusion_amd.embeddings import load_embed
    (tmp_path / "corrupt.pt").write_bytes(b"not a checkpoint at all" * 10)
    (tmp_path / "corrupt2.safetensors").write_bytes(b"\xff" * 64)
    marker = str(tmp_path / "executed")
    torch.save({"clip_l": _NeedsUnpickling(marker)}, tmp_path / "evil.pt")
    for name in ("corrupt", "corrupt2", "evil"):
        caplog.clear()
        with caplog.at_level(logging.WARNING):
            assert load_embed(name, str(tmp_path), 8) is None
        assert any(r.levelno == logging.WARNING and name in r.getMessage() for r in caplog.records), name
    assert not os.path.exists(marker), "the pickle's code ran"


# ------------------------------------------------------------------ tokenizer
def test_tokenizer_chunks_match_the_reference(gold, emb_dir):
    """fails without the feature: `embedding:three` would go through BPE as a word (here: a KeyError of the word map)"""
    tok = tokenizer(gold, emb_dir)
    assert len(gold["prompts"]) >= 10
    for key, p in gold["prompts"].items():
        got = tok.tokenize_with_weights(p["prompt"])
        assert [[[slot(gold, t), w] for t, w in c] for c in got] == p["chunks"], key
        assert all(len(c) == 77 for c in got), key
    # the chunking cases, stated: a 3-row group moves whole into chunk 2; a 10-row group ("large") is cut where the chunk ends
    ch = gold["prompts"]["filler75_three_moves"]["chunks"]
    assert [t for t, _ in ch[1][1:4]] == [["e", "three", r] for r in range(3)] and not any(isinstance(t, list) for t, _ in ch[0])
    ch = gold["prompts"]["filler70_ten_splits"]["chunks"]
    assert [t for t, _ in ch[0][71:76]] == [["e", "ten", r] for r in range(5)] and [t for t, _ in ch[1][1:6]] == [["e", "ten", r] for r in range(5, 10)]


def test_missing_embedding_warns_and_is_dropped(gold, emb_dir, caplog):
    seen = []
    from lightdiffusion_amd.clip import PromptTokenizer
    tok = PromptTokenizer(lambda w: seen.append(w) or [7], embedding_directory=emb_dir, embedding_size=64)
    with caplog.at_level(logging.WARNING):
        chunks = tok.tokenize_with_weights("a embedding:nothere, cat")
    assert any("nothere" in r.getMessage() for r in caplog.records)
    assert seen == ["a", ",", "cat"]                       # the name is never BPE'd; the comma left over after the retry is a word
    assert [t for t, _ in chunks[0][:5]] == [49406, 7, 7, 7, 49407]


def test_without_a_directory_the_tokenizer_is_unchanged(gold):
    from lightdiffusion_amd.clip import PromptTokenizer
    word_ids = lambda w: [100 + zlib.crc32(f"{w}#{i}".encode()) % 40000 for i in range(1 + len(w) // 4)]
    for tok in (PromptTokenizer(word_ids), PromptTokenizer(word_ids, embedding_directory=None, embedding_size=64)):
        for text, want in json.load(open(os.path.join(GOLDEN, "token_chunks.json"))).items():
            assert [[list(p) for p in c] for c in tok.tokenize_with_weights(text)] == want, text
        got = tok.tokenize_with_weights("a embedding:three cat")           # an ordinary word, as before
        want = [49406] + word_ids("a") + word_ids("embedding:three") + word_ids("cat") + [49407]
        assert [t for t, _ in got[0][:len(want)]] == want


# ------------------------------------------------------------------ id remap and side table
class RecordingTextModel:
    """stands in for CLIPTextModelHIP: records what CLIP hands it"""

    def __init__(self, cfg):
        self.cfg, self.calls = cfg, []

    def __call__(self, tokens, intermediate_output=None, extra_embeds=None):
        self.calls.append((tokens, extra_embeds))
        B, L = tokens.shape
        h = self.cfg["hidden_size"]
        return torch.zeros(B, L, h), None, torch.zeros(B, h)


def test_id_remap_and_side_table_match_the_reference(gold, emb_dir, caplog):
    from lightdiffusion_amd.clip import CLIP
    tok = tokenizer(gold, emb_dir)
    for key, p in gold["prompts"].items():
        tm = RecordingTextModel(gold["config"])
        with caplog.at_level(logging.WARNING):
            caplog.clear()
            cond, pooled = CLIP(tm, tok).encode_from_tokens(tok.tokenize_with_weights(p["prompt"]), return_pooled=True)
        (tokens, extra), = tm.calls
        assert tokens.dtype == torch.long and tokens.tolist() == p["ids"], key
        assert extra.dtype == torch.float32 and [slot(gold, r) for r in extra] == p["side_table"], key
        assert cond.shape == (1, 77 * len(p["chunks"]), 64) and pooled.shape == (1, 64)
        if key == "wrong_width_pad_quirk":
            assert any("96 != 64" in r.getMessage() for r in caplog.records)
    V = gold["config"]["vocab_size"]
    w = gold["prompts"]["weighted"]["ids"]
    assert len(w) == 2 and w[1] == [49406] + [V - 1 + 3] * 76           # the empty row rides along, its EOS remapped with the rest
    q = gold["prompts"]["wrong_width_pad_quirk"]["ids"][0]
    assert q[-2:] == [V - 1, V - 1] and q[3:6] == [V - 1, V, V + 1]      # the quirk: the literal pad id is the first custom vector's id


def test_prompt_without_vectors_calls_the_text_model_as_before():
    from lightdiffusion_amd.clip import CLIP
    seen = []

    def text_model(tokens, intermediate_output=None):               # the old protocol: no extra_embeds argument
        seen.append(tokens)
        return torch.zeros(*tokens.shape, 8), None, torch.zeros(tokens.shape[0], 8)
    ids = [49406, 5, 6] + [49407] * 74
    CLIP(text_model).encode_from_tokens([[(t, 1.0) for t in ids]])
    assert seen[0].tolist() == [ids]
