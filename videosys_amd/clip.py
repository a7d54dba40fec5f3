"""CLIP text encoders on MI355X — the two ``CLIPTextModelWithProjection`` objects Vchitect-2.0 runs once per prompt (transformers
modeling_clip.py, third-party; loaded at pipeline_vchitect.py:194-201, called at :333-386): CLIP-L (12 layers x 768, quick_gelu) and
CLIP-bigG (32 layers x 1280, gelu), both with 64-wide heads, 77 positions and a causal mask.  State-dict keys are the HF ones
(``text_model.embeddings.{token,position}_embedding.weight``, ``text_model.encoder.layers.N.{self_attn.{q,k,v,out}_proj, layer_norm1,
mlp.fc1, mlp.fc2, layer_norm2}.{weight,bias}``, ``text_model.final_layer_norm.*``, ``text_projection.weight``).

Per layer: LayerNorm -> fused q|k|v linear (+ bias) -> causal attention (vsys_clip_attention_d64) -> out_proj (+ bias, + residual)
-> LayerNorm -> fc1 (+ bias, activation) -> fc2 (+ bias, + residual).  77 rows against 0.1 - 0.7 B weights: like T5 the encoder is a
weight stream, so every linear is the weight-streaming GEMM of ops.linear_skinny (rows padded to 384, clip_ops.py) and its split-K finish carries
the bias, the activation and the residual (vsys_splitk_reduce_bias_act).  Token embedding and the pooled row are vsys_gather_rows,
the position embedding vsys_add_bcast_rows, the LayerNorms vsys_ln_modulate without modulation.  No CPU path."""
from __future__ import annotations

from types import SimpleNamespace
from typing import Dict

import torch

from . import clip_ops, ops
from .workspace import Workspace

ACTS = {"quick_gelu": clip_ops.ACT_QUICK_GELU, "gelu": clip_ops.ACT_GELU}
CLIP_L = dict(hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12, vocab_size=49408,
              max_position_embeddings=77, hidden_act="quick_gelu", projection_dim=768, eos_token_id=2)
CLIP_BIGG = dict(hidden_size=1280, intermediate_size=5120, num_hidden_layers=32, num_attention_heads=20, vocab_size=49408,
                 max_position_embeddings=77, hidden_act="gelu", projection_dim=1280, eos_token_id=2)
_LAYER_PARTS = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.out_proj", "layer_norm1", "mlp.fc1", "mlp.fc2",
                "layer_norm2")


def state_dict_keys(num_hidden_layers: int):
    """The keys load_state_dict reads: those of ``CLIPTextModelWithProjection(config).state_dict()``."""
    keys = ["text_model.embeddings.token_embedding.weight", "text_model.embeddings.position_embedding.weight"]
    for i in range(num_hidden_layers):
        keys += [f"text_model.encoder.layers.{i}.{p}.{wb}" for p in _LAYER_PARTS for wb in ("weight", "bias")]
    return keys + ["text_model.final_layer_norm.weight", "text_model.final_layer_norm.bias", "text_projection.weight"]


def pooled_positions(input_ids: torch.Tensor, eos_token_id: int) -> torch.Tensor:
    """[B] int64: the position whose hidden state CLIPTextTransformer pools (transformers modeling_clip.py) — with the legacy
    ``eos_token_id == 2`` config (the one SD3's checkpoints carry) the argmax of the ids, else the first position equal to
    ``eos_token_id`` (position 0 when there is none, as argmax over an all-zero row gives)."""
    ids = input_ids.to(torch.int64)
    if eos_token_id == 2:
        return ids.argmax(dim=-1)
    return (ids == eos_token_id).to(torch.int64).argmax(dim=-1)


class CLIPTextOutput:
    """What ``CLIPTextModelWithProjection.forward`` returns, as far as callers read it: ``out[0]`` / ``.text_embeds`` the pooled
    projection, ``.last_hidden_state`` (after final_layer_norm), ``.hidden_states`` (embeddings + every layer, the last one BEFORE
    final_layer_norm; None unless asked for)."""

    def __init__(self, text_embeds, last_hidden_state, hidden_states):
        self.text_embeds, self.last_hidden_state, self.hidden_states = text_embeds, last_hidden_state, hidden_states

    def __getitem__(self, i):
        return tuple(v for v in (self.text_embeds, self.last_hidden_state, self.hidden_states) if v is not None)[i]


class CLIPTextEncoder:
    def __init__(self, hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12, vocab_size=49408,
                 max_position_embeddings=77, hidden_act="quick_gelu", projection_dim=768, eos_token_id=2, layer_norm_eps=1e-5,
                 device="cuda"):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("videosys_amd.CLIPTextEncoder needs a HIP device (no CPU path)")
        if hidden_size != 64 * num_attention_heads:
            raise ValueError(f"hidden_size {hidden_size} != 64 * num_attention_heads ({num_attention_heads}): the attention kernel is "
                             "built for head dim 64 (CLIP-L and CLIP-bigG)")
        if hidden_act not in ACTS:
            raise ValueError(f"hidden_act {hidden_act!r}: expected 'quick_gelu' or 'gelu'")
        if intermediate_size % 32 or projection_dim % 8 or hidden_size > 3072:
            raise ValueError("intermediate_size must be a multiple of 32, projection_dim of 8, hidden_size at most 3072")
        if max_position_embeddings > 128:
            raise ValueError("max_position_embeddings above 128: the attention kernel holds a whole row of logits in registers")
        self.config = SimpleNamespace(hidden_size=hidden_size, intermediate_size=intermediate_size, num_hidden_layers=num_hidden_layers,
                                      num_attention_heads=num_attention_heads, vocab_size=vocab_size,
                                      max_position_embeddings=max_position_embeddings, hidden_act=hidden_act,
                                      projection_dim=projection_dim, eos_token_id=eos_token_id, layer_norm_eps=layer_norm_eps)
        self.device, self.dtype = dev, torch.bfloat16
        self.w: Dict[str, torch.Tensor] = {}
        self._ws = Workspace(dev)
        self.launches = 0     # kernel launches of the last forward (tools/clip_bench.py)

    # ------------------------------------------------------------------------------------------------ weights
    def load_state_dict(self, sd: Dict[str, torch.Tensor]):
        c = self.config
        missing = [k for k in state_dict_keys(c.num_hidden_layers) if k not in sd]
        if missing:
            raise KeyError(f"missing keys: {missing[:8]}{'...' if len(missing) > 8 else ''}")
        dev = lambda t: t.detach().to(device=self.device, dtype=self.dtype).contiguous()
        w = self.w
        w["tok"] = dev(sd["text_model.embeddings.token_embedding.weight"])
        w["pos"] = dev(sd["text_model.embeddings.position_embedding.weight"])
        for i in range(c.num_hidden_layers):
            p = f"text_model.encoder.layers.{i}."
            for wb in ("weight", "bias"):
                w[f"{i}.qkv.{wb}"] = dev(torch.cat([sd[p + f"self_attn.{n}_proj.{wb}"] for n in "qkv"], 0))
                for ours, theirs in (("o", "self_attn.out_proj"), ("ln1", "layer_norm1"), ("fc1", "mlp.fc1"), ("fc2", "mlp.fc2"),
                                     ("ln2", "layer_norm2")):
                    w[f"{i}.{ours}.{wb}"] = dev(sd[p + f"{theirs}.{wb}"])
        w["ln_f.weight"], w["ln_f.bias"] = dev(sd["text_model.final_layer_norm.weight"]), dev(sd["text_model.final_layer_norm.bias"])
        w["proj"] = dev(sd["text_projection.weight"])
        self._check_shapes()
        return self

    def _check_shapes(self):
        c, w = self.config, self.w
        C, F = c.hidden_size, c.intermediate_size
        want = {"tok": (c.vocab_size, C), "pos": (c.max_position_embeddings, C), "proj": (c.projection_dim, C), "ln_f.weight": (C,)}
        for i in range(c.num_hidden_layers):
            want.update({f"{i}.qkv.weight": (3 * C, C), f"{i}.qkv.bias": (3 * C,), f"{i}.o.weight": (C, C), f"{i}.fc1.weight": (F, C),
                         f"{i}.fc1.bias": (F,), f"{i}.fc2.weight": (C, F), f"{i}.fc2.bias": (C,)})
        for k, s in want.items():
            if tuple(w[k].shape) != s:
                raise ValueError(f"{k}: shape {tuple(w[k].shape)}, the config asks for {s}")

    def init_random_(self, seed: int = 0):
        """Random weights generated ON the device (synthetic pipelines and benchmarks: no host copy of 0.7 B parameters)."""
        c, dev = self.config, self.device
        g = torch.Generator(device=dev).manual_seed(seed)
        r = lambda *s, scale=1.0: (torch.randn(*s, generator=g, device=dev) * scale).to(self.dtype)
        C, F, w = c.hidden_size, c.intermediate_size, self.w
        w["tok"], w["pos"] = r(c.vocab_size, C, scale=0.02), r(c.max_position_embeddings, C, scale=0.01)
        for i in range(c.num_hidden_layers):
            w[f"{i}.qkv.weight"], w[f"{i}.qkv.bias"] = r(3 * C, C, scale=C ** -0.5), r(3 * C, scale=0.02)
            w[f"{i}.o.weight"], w[f"{i}.o.bias"] = r(C, C, scale=C ** -0.5), r(C, scale=0.02)
            w[f"{i}.fc1.weight"], w[f"{i}.fc1.bias"] = r(F, C, scale=C ** -0.5), r(F, scale=0.02)
            w[f"{i}.fc2.weight"], w[f"{i}.fc2.bias"] = r(C, F, scale=F ** -0.5), r(C, scale=0.02)
            for ln in ("ln1", "ln2"):
                w[f"{i}.{ln}.weight"], w[f"{i}.{ln}.bias"] = (1 + r(C, scale=0.1).float()).to(self.dtype), r(C, scale=0.02)
        w["ln_f.weight"], w["ln_f.bias"] = (1 + r(C, scale=0.1).float()).to(self.dtype), r(C, scale=0.02)
        w["proj"] = r(c.projection_dim, C, scale=C ** -0.5)
        return self

    # ------------------------------------------------------------------------------------------------ forward
    @torch.no_grad()
    def forward(self, input_ids: torch.Tensor, output_hidden_states: bool = False, **_ignored) -> CLIPTextOutput:
        c, w, buf = self.config, self.w, self._ws.buf
        if not w:
            raise RuntimeError("CLIPTextEncoder: no weights (load_state_dict or init_random_ first)")
        B, L = input_ids.shape
        if L < 1 or L > c.max_position_embeddings:
            raise ValueError(f"sequence length {L}: expected 1 .. max_position_embeddings = {c.max_position_embeddings}")
        C, F, H = c.hidden_size, c.intermediate_size, c.num_attention_heads
        M = B * L
        Mp = (M + 383) // 384 * 384        # the 256 x 384 tile of the weight-streaming linears; rows >= M never reach a result
        act, eps = ACTS[c.hidden_act], c.layer_norm_eps
        ids = input_ids.reshape(-1).to(device=self.device, dtype=torch.int64).contiguous()
        # pooled row b * L + pos: integer ops on the ids, on the device
        pool = (pooled_positions(ids.view(B, L), c.eos_token_id) + torch.arange(B, device=self.device) * L).contiguous()
        x, h, ao = buf("clip_x", (Mp, C)), buf("clip_h", (Mp, C)), buf("clip_ao", (Mp, C))
        qkv, f = buf("clip_qkv", (Mp, 3 * C)), buf("clip_f", (Mp, F))
        shapes = ((3 * C, C), (C, C), (F, C), (C, F), (c.projection_dim, C))
        part = buf("clip_part", (max(ops.skinny_split(n, Mp, k, True) * n * Mp for n, k in shapes),), torch.float32)
        lin = clip_ops.linear_skinny_bias_act
        ops.gather_rows(w["tok"], ids, out=x[:M])
        ops.add_bcast_rows(x[:M], w["pos"], 1, L)
        hs = [x[:M].view(B, L, C).clone()] if output_hidden_states else None
        for i in range(c.num_hidden_layers):
            ops.ln_modulate(x[:M], w[f"{i}.ln1.weight"], w[f"{i}.ln1.bias"], None, None, L, eps=eps, out=h[:M])
            lin(h, M, w[f"{i}.qkv.weight"], bias=w[f"{i}.qkv.bias"], out=qkv, part=part)
            clip_ops.clip_attention64(qkv, B, L, H, out=ao)
            lin(ao, M, w[f"{i}.o.weight"], bias=w[f"{i}.o.bias"], res=x, out=x, part=part)
            ops.ln_modulate(x[:M], w[f"{i}.ln2.weight"], w[f"{i}.ln2.bias"], None, None, L, eps=eps, out=h[:M])
            lin(h, M, w[f"{i}.fc1.weight"], bias=w[f"{i}.fc1.bias"], act=act, out=f, part=part)
            lin(f, M, w[f"{i}.fc2.weight"], bias=w[f"{i}.fc2.bias"], res=x, out=x, part=part)
            if output_hidden_states:
                hs.append(x[:M].view(B, L, C).clone())
        last = torch.empty(M, C, dtype=self.dtype, device=self.device)
        ops.ln_modulate(x[:M], w["ln_f.weight"], w["ln_f.bias"], None, None, L, eps=eps, out=last)
        ops.gather_rows(last, pool, out=h[:B])
        embeds = torch.empty(B, c.projection_dim, dtype=self.dtype, device=self.device)
        lin(h, B, w["proj"], out=embeds, part=part)
        self.launches = 2 + 11 * c.num_hidden_layers + 4   # embedding 2, 11 per layer, final LN + pooled gather + projection (2)
        return CLIPTextOutput(embeds, last.view(B, L, C), tuple(hs) if hs is not None else None)

    __call__ = forward


class _Encoding(dict):
    """``tokenizer(...)``'s result: a dict whose entries also read as attributes (``.input_ids``), like transformers' BatchEncoding."""

    __getattr__ = dict.__getitem__


class ClipByteTokenizer:
    """Offline stand-in for ``CLIPTokenizer`` in ``text_encoder="synthetic:<seed>"`` pipelines (the BPE vocabulary cannot be fetched
    here), as t5.ByteTokenizer is for T5: id 1 (begin), the UTF-8 bytes + 2, the end token, then padding with id 0.  The end token is
    the LARGEST id (``vocab_size - 1``), so both pooling rules of CLIPTextTransformer find it: the argmax of the ids and the first
    position equal to ``eos_token_id``."""

    model_max_length = 77
    pad_token_id, bos_token_id, byte_offset = 0, 1, 2

    def __init__(self, vocab_size: int = 49408):
        if vocab_size < 256 + 3:
            raise ValueError(f"vocab_size {vocab_size}: the byte tokenizer needs 256 byte ids and three specials")
        self.vocab_size = vocab_size
        self.eos_token_id = vocab_size - 1

    def _encode(self, text, limit):
        body = [v + self.byte_offset for v in text.encode("utf-8")]
        if limit is not None:
            body = body[: max(limit - 2, 0)]
        return [self.bos_token_id] + body + [self.eos_token_id]

    def __call__(self, prompts, padding=False, max_length=None, truncation=False, return_tensors="pt", **_ignored):
        if isinstance(prompts, str):
            prompts = [prompts]
        limit = (max_length or self.model_max_length) if truncation else None
        toks = [self._encode(p, limit) for p in prompts]
        if padding == "max_length":
            width = max_length or self.model_max_length
            if any(len(t) > width for t in toks):
                raise ValueError(f"a prompt is longer than max_length = {width} and truncation is off")
        elif padding in ("longest", True):
            width = max(len(t) for t in toks)
        elif len({len(t) for t in toks}) == 1:
            width = len(toks[0])
        else:
            raise ValueError("prompts of different lengths need padding='longest' or 'max_length'")
        ids = torch.full((len(toks), width), self.pad_token_id, dtype=torch.int64)
        mask = torch.zeros(len(toks), width, dtype=torch.int64)
        for b, t in enumerate(toks):
            ids[b, : len(t)] = torch.tensor(t)
            mask[b, : len(t)] = 1
        return _Encoding(input_ids=ids, attention_mask=mask)

    def batch_decode(self, ids, skip_special_tokens: bool = True):
        out = []
        for row in torch.as_tensor(ids).tolist():
            body = bytes(v - self.byte_offset for v in row if self.byte_offset <= v < self.byte_offset + 256)
            out.append(body.decode("utf-8", errors="replace"))
        return out


def synth_state_dict(hidden_size=768, intermediate_size=3072, num_hidden_layers=12, vocab_size=49408, max_position_embeddings=77,
                     projection_dim=768, seed: int = 5):
    """Seeded random weights with the HF CLIPTextModelWithProjection key names (bf16-representable fp32)."""
    g = torch.Generator().manual_seed(seed)
    C, F = hidden_size, intermediate_size
    r = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(torch.bfloat16).float()
    one = lambda n: (1 + r(n, scale=0.1)).to(torch.bfloat16).float()
    sd = {"text_model.embeddings.token_embedding.weight": r(vocab_size, C, scale=0.5),
          "text_model.embeddings.position_embedding.weight": r(max_position_embeddings, C, scale=0.25)}
    for i in range(num_hidden_layers):
        p = f"text_model.encoder.layers.{i}."
        for n in ("q", "k", "v", "out"):
            sd[p + f"self_attn.{n}_proj.weight"], sd[p + f"self_attn.{n}_proj.bias"] = r(C, C, scale=C ** -0.5), r(C, scale=0.1)
        sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"] = r(F, C, scale=C ** -0.5), r(F, scale=0.1)
        sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"] = r(C, F, scale=F ** -0.5), r(C, scale=0.1)
        for ln in ("layer_norm1", "layer_norm2"):
            sd[p + ln + ".weight"], sd[p + ln + ".bias"] = one(C), r(C, scale=0.1)
    sd["text_model.final_layer_norm.weight"], sd["text_model.final_layer_norm.bias"] = one(C), r(C, scale=0.1)
    sd["text_projection.weight"] = r(projection_dim, C, scale=C ** -0.5)
    return sd
