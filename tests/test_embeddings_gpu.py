"""GPU: the CLIP input-stage kernel (ld_op_clip_embed) bit for bit against the torch expression it replaces, and textual-inversion prompts end
to end against the reference's recorded conditioning (tools/make_embedding_golden.py)."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden, rel_l2
from embedding_files import write_embedding_files

pytestmark = pytest.mark.gpu
# the kernel of clip.hip and the tests that hold it bitwise (tests/test_errbound_cpu.py keeps the ledger)
KERNELS = {"clip_embed_kernel": ["test_clip_embed_kernel_bitwise", "test_clip_embed_every_id_class_in_one_row"]}
DEV = "cuda:0"
E2E_BOUND = 5e-3           # this text model against the reference: tests/test_models_gpu.py::test_clip_text_model_on_hip_kernels
V_CLIP = 49408


def torch_embed(ids, table, pos, extra=None):
    """the expression CLIPTextModelHIP used before the kernel — (table[ids].float() + pos.float()).half() — with rows V-1 .. V-2+E taken from
    the fp32 side table and V-1+E from the EOS row, without building the [V + E, h] table"""
    V, E = table.shape[0], 0 if extra is None else extra.shape[0]
    ids = ids.to(table.device)
    rows = table[torch.where(ids >= V - 1 + E, ids - E, ids).clamp(0, V - 1)].float()
    if E:
        custom = (ids >= V - 1) & (ids < V - 1 + E)
        rows = torch.where(custom[..., None], extra[(ids - (V - 1)).clamp(0, E - 1)], rows)
    return (rows + pos[:ids.shape[1]].float()).half()


@pytest.fixture(scope="module")
def tables():
    g = torch.Generator(device="cpu").manual_seed(5)
    out = {}
    for h in (64, 768):
        table = (0.5 * torch.randn(V_CLIP, h, generator=g)).half().to(DEV)
        pos = (0.5 * torch.randn(77, h, generator=g)).half().to(DEV)
        extra = (0.5 * torch.randn(10, h, generator=g)).to(DEV)
        out[h] = (table, pos, extra)
    return out


@pytest.mark.parametrize("h", [64, 768])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("E", [0, 1, 10])
def test_clip_embed_kernel_bitwise(tables, h, B, E):
    from lightdiffusion_amd import ops
    table, pos, extra10 = tables[h]
    extra = extra10[:E].contiguous() if E else None
    V, L = V_CLIP, 77
    ids = torch.randint(0, V + E, (B, L), generator=torch.Generator().manual_seed(100 * B + E))
    ids[:, 0] = 49406
    ids[0, 1:6] = torch.tensor([0, V - 2, V - 1, V - 2 + E, V - 1 + E])     # both boundaries of the custom range, every class
    ids[-1, 40:] = V - 1 + E
    out, dev_ids = ops.clip_embed(ids.tolist(), table, pos, extra)
    assert out.shape == (B, L, h) and out.dtype == torch.float16 and dev_ids.dtype == torch.int32 and dev_ids.cpu().tolist() == ids.tolist()
    assert torch.equal(out, torch_embed(ids, table, pos, extra))
    if E == 0:
        assert torch.equal(out, (table[ids.to(DEV)].float() + pos.float()).half())        # the line the kernel replaces, as it stood


def test_clip_embed_every_id_class_in_one_row():
    from lightdiffusion_amd import ops
    V, L, E, h = 16, 5, 3, 64
    g = torch.Generator().manual_seed(6)
    table, pos, extra = torch.randn(V, h, generator=g).half().to(DEV), torch.randn(7, h, generator=g).half().to(DEV), torch.randn(E, h, generator=g).to(DEV)
    ids = [[3, V - 2, V - 1, V - 2 + E, V - 1 + E]]
    out, _ = ops.clip_embed(ids, table, pos, extra)
    want = torch.stack([table[3].float(), table[V - 2].float(), extra[0], extra[E - 1], table[V - 1].float()])
    assert torch.equal(out[0], (want + pos[:L].float()).half())
    assert torch.equal(out, torch_embed(torch.tensor(ids), table, pos, extra))
    out0, _ = ops.clip_embed([[3, V - 2, V - 1, 0, 1]], table, pos, None)             # E = 0: V-1 is EOS itself
    assert torch.equal(out0[0, 2], (table[V - 1].float() + pos[2].float()).half())


def test_clip_embed_refuses_shapes_and_ids_without_launching():
    from lightdiffusion_amd import ops
    from lightdiffusion_amd._lib import ERR_ARG, ERR_SHAPE, LDError, lib
    V, L, h = 16, 5, 12
    table, pos = torch.ones(V, h, dtype=torch.float16, device=DEV), torch.ones(L, h, dtype=torch.float16, device=DEV)
    ids = torch.zeros(1, L, dtype=torch.int32, device=DEV)
    out = torch.full((1, L, h), 7.0, dtype=torch.float16, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    assert lib().ld_op_clip_embed(ids.data_ptr(), table.data_ptr(), None, pos.data_ptr(), out.data_ptr(), 1, L, V, 0, h, stream) == ERR_SHAPE
    assert lib().ld_op_clip_embed(ids.data_ptr(), None, None, pos.data_ptr(), out.data_ptr(), 1, L, V, 0, 16, stream) == ERR_ARG
    assert lib().ld_op_clip_embed(ids.data_ptr(), table.data_ptr(), None, pos.data_ptr(), out.data_ptr(), 1, L, V, 2, 16, stream) == ERR_ARG   # E > 0, no side table
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), "a refused call wrote its output"
    with pytest.raises(LDError) as e:
        ops.clip_embed([[0] * L], table, pos)
    assert e.value.status == ERR_SHAPE
    table, pos = torch.ones(V, 16, dtype=torch.float16, device=DEV), torch.ones(L, 16, dtype=torch.float16, device=DEV)
    with pytest.raises(LDError) as e:
        ops.clip_embed([[0] * (L + 1)], table, pos)                     # more tokens per row than the position table has rows
    assert e.value.status == ERR_SHAPE
    extra = torch.ones(2, 16, device=DEV)
    for bad, ex in ((V, None), (-1, None), (V + 2, extra), (1 << 40, extra)):       # checked on the host, before anything is uploaded
        with pytest.raises(ValueError):
            ops.clip_embed([[0, 1, bad, 2, 3]], table, pos, ex)
    assert ops.clip_embed([[0, 1, V + 1, 2, 3]], table, pos, extra)[0].shape == (1, L, 16)


def test_text_model_without_vectors_is_bit_identical_to_the_expression_path():
    from lightdiffusion_amd import weights as W
    from lightdiffusion_amd.clip import CLIPTextModelHIP
    g = load_golden("clip_tiny")
    cfg = W.tiny_clip_config()
    tm = CLIPTextModelHIP(cfg, W.synth_state_dict(W.clip_param_shapes(cfg)), device=DEV)
    got = tm(g["tokens"], intermediate_output=-2)
    tokens = g["tokens"].to(DEV)
    P = "text_model.embeddings."
    x = (tm.w[P + "token_embedding.weight"][tokens].float() + tm.w[P + "position_embedding.weight"].float()).half().contiguous()
    with torch.no_grad():
        want = tm._encode(x, tokens, -2)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert rel_l2(got[0].cpu(), g["last"]) < E2E_BOUND


@pytest.fixture(scope="module")
def gold():
    g = json.load(open(os.path.join(GOLDEN, "embeddings.json")))
    with np.load(os.path.join(GOLDEN, "embeddings.npz")) as z:
        g["vectors"] = {n: torch.from_numpy(z["vec_" + n]) for n in g["files"]}
        g["arrays"] = {k: torch.from_numpy(z[k]) for k in z.files if not k.startswith("vec_")}
    return g


def test_embedding_prompts_end_to_end_against_the_reference(gold, tmp_path):
    from lightdiffusion_amd import weights as W
    from lightdiffusion_amd.clip import CLIP, CLIPTextModelHIP, PromptTokenizer
    cfg = W.tiny_clip_config()
    assert cfg == gold["config"]
    emb_dir = write_embedding_files(str(tmp_path), gold["vectors"])
    tok = PromptTokenizer(lambda w: gold["word_ids"][w], embedding_directory=emb_dir, embedding_size=cfg["hidden_size"])
    clip = CLIP(CLIPTextModelHIP(cfg, W.synth_state_dict(W.clip_param_shapes(cfg)), device=DEV), tok)
    assert len(gold["prompts"]) >= 10
    failed = []
    for key, p in gold["prompts"].items():
        # a result that ignored the embedding words would sit at least 10 bounds away from the reference's
        assert p["deleted_rel_l2"] >= 10 * E2E_BOUND, key
        cond, pooled = clip.encode_from_tokens(tok.tokenize_with_weights(p["prompt"]), return_pooled=True)
        want_c, want_p = gold["arrays"]["cond_" + key], gold["arrays"]["pooled_" + key]
        assert cond.shape == want_c.shape and pooled.shape == want_p.shape, key
        ec, ep = rel_l2(cond, want_c), rel_l2(pooled, want_p)
        print(f"{key}: cond rel-L2 {ec:.2e}, pooled rel-L2 {ep:.2e} (without the embedding words: {p['deleted_rel_l2']:.2e})")
        if not (ec < E2E_BOUND and ep < E2E_BOUND):
            failed.append((key, ec, ep))
    assert not failed, failed


def test_no_vocabulary_sized_copy_per_prompt(tmp_path):
    """The reference rebuilds a [V + E, 768] table per prompt (76 MB in fp16); here an encode with 10 custom vectors may grow the peak by less
    than half of that."""
    from lightdiffusion_amd import weights as W
    from lightdiffusion_amd.clip import CLIP, CLIPTextModelHIP, PromptTokenizer
    cfg = W.sd15_clip_config()
    torch.save({"clip_l": W.synth_tensor("embeddings.ten768.token_embedding.weight", (10, 768))}, tmp_path / "ten768.pt")
    tok = PromptTokenizer(lambda w: [1000 + len(w)], embedding_directory=str(tmp_path), embedding_size=768)
    clip = CLIP(CLIPTextModelHIP(cfg, W.synth_state_dict(W.clip_param_shapes(cfg), dtype=torch.float16), device=DEV), tok)
    clip.encode_from_tokens(tok.tokenize_with_weights("a photo of a cat"))                   # warm-up: the operators' cached scratch
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    chunks = tok.tokenize_with_weights("a photo of embedding:ten768 cat")
    assert sum(isinstance(t, torch.Tensor) for t, _ in chunks[0]) == 10
    cond = clip.encode_from_tokens(chunks)
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - before
    print(f"peak growth of an encode with 10 custom vectors: {growth / 1e6:.2f} MB")
    assert cond.shape == (1, 77, 768) and torch.isfinite(cond).all()
    assert growth < 38e6, growth
