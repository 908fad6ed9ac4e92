"""CLIP-L text conditioning: prompt-weight parsing, 77-token chunking, the 12-layer causal text
transformer (on the HIP kernels through the C ABI: `CLIPTextModelHIP`, the package's only text model) and the per-token weight
lerp.  Runs once per prompt; its output is the payload of the one RCCL broadcast.

Mirrors: token_weights / parse_parentheses (LD.py:4733-4780), SDTokenizer.tokenize_with_weights (LD.py:4936-5031),
ClipTokenWeightEncoder.encode_token_weights (LD.py:4540-4569), SDClipModel.forward (LD.py:4692-4724),
CLIPTextModel_ (LD.py:4413-4463), CLIP.tokenize / encode_from_tokens / clip_layer (LD.py:6222-6272).
"""
from __future__ import annotations

import logging
from typing import Callable, Dict, List, Optional, Sequence, Tuple, Union

import torch

START_TOKEN, END_TOKEN = 49406, 49407
_ESC_CLOSE, _ESC_OPEN = "\0\1", "\0\2"


# ------------------------------------------------------------------ "(text:1.2)" emphasis syntax
def _split_top_level_groups(text: str) -> List[str]:
    """Cut `text` at top-level parenthesis groups: a cut before a '(' seen at depth 0 and after the ')' that returns the
    depth to 0.  Depth may go negative on stray ')' (then nothing closes until it is back at 0) — same as the reference."""
    pieces, start, depth = [], 0, 0
    for i, ch in enumerate(text):
        if ch == "(":
            if depth == 0 and i > start:
                pieces.append(text[start:i])
                start = i
            depth += 1
        elif ch == ")":
            depth -= 1
            if depth == 0:
                pieces.append(text[start:i + 1])
                start = i + 1
    if start < len(text):
        pieces.append(text[start:])
    return pieces


def parse_prompt_weights(text: str, base: float = 1.0) -> List[Tuple[str, float]]:
    """(segment, weight) list.  A "( ... )" group multiplies the weight by 1.1, or sets it to the number after the
    group's last ':' when that parses as a float; groups nest."""
    out: List[Tuple[str, float]] = []
    for piece in _split_top_level_groups(text):
        if len(piece) >= 2 and piece[0] == "(" and piece[-1] == ")":
            inner, w = piece[1:-1], base * 1.1
            colon = inner.rfind(":")
            if colon > 0:
                try:
                    w, inner = float(inner[colon + 1:]), inner[:colon]
                except ValueError:
                    pass
            out.extend(parse_prompt_weights(inner, w))
        else:
            out.append((piece, base))
    return out


def escape_important(text: str) -> str:
    return text.replace("\\)", _ESC_CLOSE).replace("\\(", _ESC_OPEN)


def unescape_important(text: str) -> str:
    return text.replace(_ESC_CLOSE, ")").replace(_ESC_OPEN, "(")


class PromptTokenizer:
    """Word-level BPE front end + the reference's chunking rules: [BOS] tokens... [EOS] padded with EOS to 77; words of
    fewer than 8 tokens are never split across chunks; longer words are split and the chunk is closed with EOS."""

    max_word_length = 8
    embedding_identifier = "embedding:"

    def __init__(self, word_tokenizer: Callable[[str], List[int]], max_length: int = 77, start_token: int = START_TOKEN,
                 end_token: int = END_TOKEN, pad_with_end: bool = True, embedding_directory=None, embedding_size: int = 768,
                 embedding_key: str = "clip_l"):
        """`embedding_directory` (a path or a list of paths; None: no textual inversion, `embedding:x` is an ordinary word) is searched with
        its sub-directories for the file a word `embedding:name` names; `embedding_size` is the text model's hidden size."""
        self.word_tokenizer = word_tokenizer
        self.max_length, self.start_token, self.end_token = max_length, start_token, end_token
        self.pad_token = end_token if pad_with_end else 0
        self.embedding_directory, self.embedding_size, self.embedding_key = embedding_directory, embedding_size, embedding_key

    @classmethod
    def from_pretrained(cls, tokenizer_dir: str, embedding_directory=None, embedding_size: int = 768,
                        embedding_key: str = "clip_l") -> "PromptTokenizer":
        """Build on HuggingFace's CLIPTokenizer files (the reference loads them from `_internal/sd1_tokenizer/`)."""
        from transformers import CLIPTokenizer
        tok = CLIPTokenizer.from_pretrained(tokenizer_dir)
        empty = tok("")["input_ids"]
        return cls(lambda w: tok(w)["input_ids"][1:-1], start_token=empty[0], end_token=empty[1], embedding_directory=embedding_directory,
                   embedding_size=embedding_size, embedding_key=embedding_key)

    def _try_get_embedding(self, name: str):
        """(vectors or None, leftover text): `name` as it stands, else with the commas around it stripped — what follows the stripped name
        is handed back to be tokenised as a word (SDTokenizer._try_get_embedding, LD.py:4917-4934)."""
        from .embeddings import load_embed
        embed = load_embed(name, self.embedding_directory, self.embedding_size, self.embedding_key)
        if embed is None:
            stripped = name.strip(",")
            if len(stripped) < len(name):
                return load_embed(stripped, self.embedding_directory, self.embedding_size, self.embedding_key), name[len(stripped):]
        return embed, ""

    def tokenize_with_weights(self, text: str) -> List[List[Tuple[Union[int, torch.Tensor], float]]]:
        """77-slot chunks of (token, weight).  A token is an id, or — for a word `embedding:name` with an embedding directory set — one
        fp32 vector of the named file: the file's rows form one group, chunked like a word's ids."""
        words: List[List[Tuple[Union[int, torch.Tensor], float]]] = []
        for seg, w in parse_prompt_weights(escape_important(text), 1.0):
            for word in unescape_important(seg).replace("\n", " ").split(" "):
                if not word:
                    continue
                if word.startswith(self.embedding_identifier) and self.embedding_directory is not None:
                    name = word[len(self.embedding_identifier):].strip("\n")
                    embed, leftover = self._try_get_embedding(name)
                    if embed is None:
                        logging.warning("embedding:%s does not exist, ignoring", name)      # dropped: never BPE'd as if it were English
                    elif embed.dim() == 1:
                        words.append([(embed, w)])
                    else:
                        words.append([(embed[r], w) for r in range(embed.shape[0])])
                    if leftover == "":
                        continue
                    word = leftover
                words.append([(t, w) for t in self.word_tokenizer(word)])
        chunks: List[List[Tuple[int, float]]] = [[(self.start_token, 1.0)]]
        cur = chunks[0]
        room = self.max_length - 1                       # slots before the closing EOS
        for group in words:
            big = len(group) >= self.max_word_length
            while group:
                if len(group) + len(cur) > room:
                    left = room - len(cur)
                    if big:
                        cur.extend(group[:left])
                        cur.append((self.end_token, 1.0))
                        group = group[left:]
                    else:
                        cur.append((self.end_token, 1.0))
                        cur.extend([(self.pad_token, 1.0)] * left)
                    cur = [(self.start_token, 1.0)]
                    chunks.append(cur)
                else:
                    cur.extend(group)
                    group = []
        cur.append((self.end_token, 1.0))
        cur.extend([(self.pad_token, 1.0)] * (self.max_length - len(cur)))
        return chunks


# ------------------------------------------------------------------ LoRA patch bookkeeping (shared by nodes.ModelPatcher and CLIP)
class LoraPatches:
    """The LoRA patches one ModelPatcher carries, and their identity: {checkpoint key: [(strength_patch, (up, down, alpha), strength_model)]}
    and a uuid that changes with every add_patches (None: the loaded weights)."""

    def __init__(self):
        self.patches: Dict[str, list] = {}
        self.uuid = None


def _add_patches(owner, model_keys, patches, strength_patch: float, strength_model: float):
    """ModelPatcher.add_patches (LD.py:3297-3307): append (strength_patch, patch, strength_model) to the list of every key of `patches` the
    model has; a new patches_uuid; returns the matched keys.  `model_keys` is {key: shape}: a patch whose name resolves but whose factors do
    not fit the weight (an SD2.x LoRA on this net: same block names, other widths) raises ValueError before anything is added, as the
    load-time merge does at its reshape — the device merge indexes the factors by the weight's rows and columns and must never see them."""
    import uuid
    from .unet import lora_factor_mismatch
    matched = [k for k in patches if k in model_keys]
    for k in matched:
        why = lora_factor_mismatch(model_keys[k], patches[k][0], patches[k][1])
        if why is not None:
            raise ValueError(f"LoRA does not fit this model: '{k}': {why}")
    for k in matched:
        owner.patches.setdefault(k, []).append((strength_patch, patches[k], strength_model))
    owner.patches_uuid = uuid.uuid4()
    return matched


def patch_terms(entries) -> list:
    """[(strength_patch, (up, down, alpha or None), strength_model)] -> [(up, down, scale)] with alpha / rank folded into the scale as
    calculate_weight does (LD.py:3407-3424: alpha *= v[2] / mat2.shape[0]; strength_model is not read there either)."""
    out = []
    for strength, (up, down, alpha), _ in entries:
        out.append((up, down, float(strength) * (float(alpha) / down.shape[0] if alpha is not None else 1.0)))
    return out


# ------------------------------------------------------------------ text transformer
class CLIPTextModelHIP:
    """CLIP-L text transformer (CLIPTextModel_, LD.py:4413-4463) on the HIP kernels — the package's ONLY text model
    (the torch CPU restatement used by host-logic tests lives in oracle/sd15_ref.py: `clip_text_model`): LayerNorm, fused [q|k|v] projection, causal
    flash attention, out-projection + residual epilogue, fc1 + quick-GELU epilogue, fc2 + residual epilogue — all through
    the C ABI (`ops`), fp16 storage / fp32 accumulation; the input stage (token gather + position add, with the prompt's textual-inversion
    vectors read from a side table) is `ops.clip_embed`.  Only the final row pick for the pooled output stays torch indexing.  The reference computes this model in fp32; the conditioning it feeds is cast to
    fp16 by `apply_model` (LD.py:5846), so the tolerance here is the per-op fp16 one."""

    def __init__(self, cfg: dict, weights: Dict[str, torch.Tensor], device="cuda:0"):
        self.cfg, self.device = dict(cfg), torch.device(device)
        self.w = {k: v.to(torch.float16).to(self.device) for k, v in weights.items()}
        P = "text_model.encoder.layers."
        self.qkv = []
        for i in range(cfg["num_hidden_layers"]):
            p = f"{P}{i}.self_attn."
            w = torch.cat([self.w[p + f"{t}_proj.weight"] for t in "qkv"]).contiguous()
            b = torch.cat([self.w[p + f"{t}_proj.bias"] for t in "qkv"]).contiguous()
            self.qkv.append((w, b))
        self._backup: Dict[str, torch.Tensor] = {}      # device clones of the LoRA-patched tensors as they were loaded
        self.applied_patches_uuid = None                # identity of the patch set merged into self.w (None: the loaded weights)

    def param_shapes(self) -> Dict[str, tuple]:
        return {k: tuple(v.shape) for k, v in self.w.items()}

    def _sync_qkv(self, key: str) -> None:
        """the fused [q|k|v] projection holds a copy of a patched q / k / v_proj weight: refresh its row block"""
        import re
        m = re.match(r"^text_model\.encoder\.layers\.(\d+)\.self_attn\.([qkv])_proj\.weight$", key)
        if m:
            h, j = self.cfg["hidden_size"], "qkv".index(m.group(2))
            self.qkv[int(m.group(1))][0][j * h:(j + 1) * h].copy_(self.w[key])

    def unpatch_weights(self, uuid=None) -> None:
        """the loaded weights back, bit for bit (ModelPatcher.unpatch_model, LD.py:3426-3437)"""
        with torch.no_grad():
            for key, saved in self._backup.items():
                self.w[key].copy_(saved)
                self._sync_qkv(key)
        self._backup = {}
        self.applied_patches_uuid = uuid

    def patch_weights(self, patches: Dict[str, list], uuid=None) -> None:
        """ModelPatcher.patch_model (LD.py:3335-3354) on the resident fp16 tensors: `patches` {key under text_model.: [(up, down, scale), ...]};
        w = round_fp16(loaded w + sum scale up down), the merge on the device (`ld_op_lora_merge`) from a device clone of the loaded tensor.
        A patch that is refused (an unknown key, factors that do not fit, a rank or a number of terms out of range) raises, and leaves the
        loaded weights in place."""
        from ._lib import check, lib
        from .unet import lora_terms
        self.unpatch_weights()
        try:
            with torch.no_grad(), torch.cuda.device(self.device):
                for key, terms in patches.items():
                    w = self.w[key]
                    if w.dim() != 2:
                        raise ValueError(f"'{key}' is not a matrix")
                    arr, keep = lora_terms(terms, self.device, tuple(w.shape))       # (ValueError unless w is a matrix the factors fit)
                    self._backup[key] = w.clone()
                    check(lib().ld_op_lora_merge(self._backup[key].data_ptr(), w.data_ptr(), w.shape[0], w.shape[1], arr, len(terms),
                                                 torch.cuda.current_stream().cuda_stream), f"ld_op_lora_merge({key})")
                    del keep
                    self._sync_qkv(key)
        except Exception:
            self.unpatch_weights()               # restores what was merged so far from its backups; applied_patches_uuid = None
            raise
        self.applied_patches_uuid = uuid if uuid is not None else object()   # (a direct call: matches no patcher, so the next lazy swap restores)

    @torch.no_grad()
    def __call__(self, tokens: torch.Tensor, intermediate_output: Optional[int] = None, extra_embeds: Optional[torch.Tensor] = None):
        """tokens [B, L] ids; `extra_embeds` [E, h] fp32: the prompt's textual-inversion vectors, selected by the ids V-1 .. V-2+E with EOS
        moved to V-1+E (CLIP.remap_textual_embeddings).  The input stage is one gather kernel on the resident table and that side table."""
        from . import ops
        P = "text_model.embeddings."
        extra = None if extra_embeds is None else extra_embeds.to(self.device, torch.float32).contiguous()
        x, tokens = ops.clip_embed(tokens, self.w[P + "token_embedding.weight"], self.w[P + "position_embedding.weight"], extra)     # [B, L, h]
        return self._encode(x, tokens, intermediate_output)

    def _encode(self, x: torch.Tensor, tokens: torch.Tensor, intermediate_output: Optional[int]):
        from . import ops
        P = "text_model."
        h, heads, nl = self.cfg["hidden_size"], self.cfg["num_attention_heads"], self.cfg["num_hidden_layers"]
        B, L = x.shape[:2]
        stop = None if intermediate_output is None else (nl + intermediate_output if intermediate_output < 0 else intermediate_output)
        inter = None
        ln = lambda t, p: ops.layer_norm(t, self.w[p + ".weight"], self.w[p + ".bias"], 1e-5)
        for i in range(nl):
            p = f"{P}encoder.layers.{i}"
            qkv = ops.linear(ln(x, p + ".layer_norm1"), *self.qkv[i])                                 # [B, L, 3h]
            q, k, v = (qkv[..., j * h:(j + 1) * h].contiguous() for j in range(3))
            a = ops.attention(q, k, v, heads, causal=True)
            x = ops.linear(a, self.w[p + ".self_attn.out_proj.weight"], self.w[p + ".self_attn.out_proj.bias"], residual=x)
            m = ops.linear(ln(x, p + ".layer_norm2"), self.w[p + ".mlp.fc1.weight"], self.w[p + ".mlp.fc1.bias"], act="quick_gelu")
            x = ops.linear(m, self.w[p + ".mlp.fc2.weight"], self.w[p + ".mlp.fc2.bias"], residual=x)
            if i == stop:
                inter = x.clone()
        x = ln(x, P + "final_layer_norm")
        if inter is not None:
            inter = ln(inter, P + "final_layer_norm")
        pooled = x[torch.arange(B, device=self.device), tokens.argmax(dim=-1)]      # the first EOS: the largest id, remapped or not
        return x.float(), None if inter is None else inter.float(), pooled.float()


class CLIP:
    """The object `CLIPTextEncode.encode(clip, text)` drives (LD.py:6222-6272)."""

    def __init__(self, text_model, tokenizer: Optional[PromptTokenizer] = None, layer_idx: Optional[int] = None):
        """text_model(tokens[B, 77] long, intermediate_output=layer_idx) -> (last hidden state, hidden state at layer_idx or None, pooled):
        `CLIPTextModelHIP` in the product.  A prompt with textual-inversion vectors also passes extra_embeds=[E, h] fp32 and needs the model's
        `cfg` (vocab_size, hidden_size) for the id remap."""
        self.text_model, self.tokenizer, self.layer_idx = text_model, tokenizer, layer_idx
        self.patches: Dict[str, list] = {}              # checkpoint key -> [(strength_patch, (up, down, alpha), strength_model)]
        self.patches_uuid = None                        # None: the loaded weights

    def clone(self) -> "CLIP":
        n = CLIP(self.text_model, self.tokenizer, self.layer_idx)
        n.patches = {k: list(v) for k, v in self.patches.items()}
        n.patches_uuid = self.patches_uuid
        return n

    # -- LoRA patches (CLIP.add_patches -> ModelPatcher.add_patches, LD.py:3297-3307): bookkeeping here, the swap is lazy (patch_model)
    KEY_PREFIX = "cond_stage_model.transformer."

    def model_key_shapes(self) -> Dict[str, tuple]:
        """{checkpoint key: shape} of the text model's parameters"""
        return {self.KEY_PREFIX + k: s for k, s in self.text_model.param_shapes().items()}

    def add_patches(self, patches, strength_patch: float = 1.0, strength_model: float = 1.0):
        return _add_patches(self, self.model_key_shapes(), patches, strength_patch, strength_model)

    def patch_model(self):
        """Make the shared resident text model carry THIS clone's patches (where the reference calls load_models_gpu, LD.py:6262): a no-op when
        they already are applied; an empty set restores the loaded weights."""
        tm = self.text_model
        if getattr(tm, "applied_patches_uuid", None) == self.patches_uuid:
            return tm
        if not hasattr(tm, "patch_weights"):
            if self.patches:
                raise RuntimeError("this text model cannot be patched (no patch_weights)")
            return tm
        if self.patches:
            tm.patch_weights({k[len(self.KEY_PREFIX):]: patch_terms(v) for k, v in self.patches.items()}, self.patches_uuid)
        else:
            tm.unpatch_weights(self.patches_uuid)
        return tm

    def unpatch_model(self):
        if hasattr(self.text_model, "unpatch_weights"):
            self.text_model.unpatch_weights()

    def clip_layer(self, layer_idx: int) -> None:           # CLIPSetLastLayer → clip skip
        self.layer_idx = layer_idx

    def tokenize(self, text: str):
        if self.tokenizer is None:
            raise RuntimeError("no tokenizer attached: build one with PromptTokenizer.from_pretrained(<sd1_tokenizer dir>)")
        return {"l": self.tokenizer.tokenize_with_weights(text)}

    def remap_textual_embeddings(self, tokens: Sequence[Sequence[Union[int, torch.Tensor]]]):
        """SDClipModel.set_up_textual_embeddings (LD.py:4642-4690) over all rows of a call, without its [V + E, h] table: (ids, side table).
        With V the rows of the token table (EOS = V-1): every accepted vector gets the id V-1, V, ... in order of appearance and a row of
        the fp32 [E, h] side table (None when E == 0); EOS becomes V-1+E, so it stays the largest id (the pooled pick is an argmax).
        A vector whose length is not h is dropped with a warning, and its row is padded at the end, back to its length, with the LITERAL
        pad id V-1.  That id is not remapped — the reference's quirk, kept as it is (its recorded conditioning decides): with E > 0 such a
        pad slot selects the first custom vector, not EOS."""
        cfg = self.text_model.cfg
        V, h = cfg["vocab_size"], cfg["hidden_size"]
        vectors, rows = [], []
        for sec in tokens:
            row = []
            for t in sec:
                if not isinstance(t, torch.Tensor):
                    row.append(-1 if t == V - 1 else int(t))
                elif t.shape[0] == h:
                    row.append(V - 1 + len(vectors))
                    vectors.append(t)
                else:
                    logging.warning("shape mismatch when trying to apply embedding, embedding will be ignored %d != %d", t.shape[0], h)
            rows.append(row + [V - 1] * (len(sec) - len(row)))
        eos = V - 1 + len(vectors)
        ids = [[eos if t == -1 else t for t in row] for row in rows]
        return ids, (torch.stack([v.to(torch.float32) for v in vectors]) if vectors else None)

    def _encode_ids(self, ids: List[List[int]], extra_embeds: Optional[torch.Tensor] = None):
        self.patch_model()
        kw = {} if extra_embeds is None else {"extra_embeds": extra_embeds}
        last, inter, pooled = self.text_model(torch.tensor(ids, dtype=torch.long), intermediate_output=self.layer_idx, **kw)
        return (last if inter is None else inter).float(), pooled.float()

    def encode_from_tokens(self, tokens, return_pooled: bool = False):
        pairs: Sequence[Sequence[Tuple[Union[int, torch.Tensor], float]]] = tokens["l"] if isinstance(tokens, dict) else tokens
        ids = [[t for t, _ in sec] for sec in pairs]
        weighted = any(w != 1.0 for sec in pairs for _, w in sec)
        n = len(ids)
        if weighted or n == 0:
            ids = ids + [[START_TOKEN, END_TOKEN] + [END_TOKEN] * (max(len(s) for s in ids) - 2 if ids else 75)]
        extra = None
        if any(isinstance(t, torch.Tensor) for sec in ids for t in sec):       # (a prompt without embedding: words keeps its ids as they are)
            ids, extra = self.remap_textual_embeddings(ids)
        out, pooled = self._encode_ids(ids, extra)
        secs = []
        for k in range(n):
            z = out[k:k + 1]
            if weighted:
                w = torch.tensor([w for _, w in pairs[k]], dtype=z.dtype, device=z.device)[None, :, None]
                z = torch.where(w != 1.0, (z - out[-1:]) * w + out[-1:], z)
            secs.append(z)
        cond = torch.cat(secs, dim=-2).cpu()                 # intermediate_device() is the CPU in the reference
        return (cond, pooled[0:1].cpu()) if return_pooled else cond
