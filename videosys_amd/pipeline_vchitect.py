"""Vchitect-2.0 pipeline plug-in — host mirror of videosys/pipelines/vchitect/pipeline_vchitect.py (VchitectPABConfig :32-55,
VchitectConfig :58-123, VchitectXLPipeline :126-997, retrieve_timesteps :1001-1057): prompt embeddings + noise -> flow-match Euler
sampling with VchitectXLTransformerModel (vchitect.py) -> SD3 VAE decode (vae_sd3.py) -> a list of PIL frames.

``VchitectConfig`` / ``VchitectPABConfig`` take the reference's keywords with its defaults and drop into ``VideoSysEngine``.

Text side.  The two CLIP encoders (CLIP-L, CLIP-bigG) are clip.CLIPTextEncoder (causal attention at head dim 64 and the
weight-streaming linears with bias and activation, clip.py): ``text_encoder`` / ``text_encoder_2`` take ``"synthetic:<seed>"``, a
local directory (config.json + model.safetensors), a torch module holding the HF weights, or any object that is called exactly as
:368-374 calls them (``enc(ids, output_hidden_states=True)``: element 0 is the pooled embedding, ``.hidden_states[-2]`` or
``[-(clip_skip + 2)]`` the prompt embedding); left at None they are read from ``<model_path>/text_encoder`` / ``text_encoder_2`` when
that is a local checkpoint, else they stay None and the caller passes ``prompt_embeds`` + ``pooled_prompt_embeds`` and the negative
pair.  ``text_encoder_3`` is this build's T5 (t5.py) at max length 256, ``None`` gives the zeros of :295-300.  Tokenizers plug in as
everywhere in this package.

Sampler.  ``FlowMatchEulerDiscreteScheduler`` below restates diffusers' class as the pipeline uses it.  One model object is called
twice per step, uncond first then text (:925-941), so VchitectAttention's PAB counters advance twice per step and the second call of a
step may broadcast what the first one computed — the reference's behaviour (one module, two calls), kept literally.  The two
predictions land in one fp32 [2, F, 16, h, w] buffer in (text, uncond) order and ``vsys_cfg_euler_step`` does the guidance combine
and the Euler update in one launch with ``dt = sigma_next - sigma``; latents stay fp32 on the device between steps.  The per-step
guidance scale is ``1 + guidance_scale * (1 - cos(pi * ((N - t) / N) ** 5)) / 2`` (:942-944) in Python doubles and is ALWAYS
applied: the reference skips the combine when that value is not above 1 and then steps with the previous step's ``noise_pred`` (a
stale local; a NameError on the first step) — that corner is not reproduced.

Batch.  The reference indexes rows 0 and 1 of the CFG pair (:925-941): it works for one prompt with guidance above 1 only.  A list
of several prompts, ``num_images_per_prompt != 1`` and ``guidance_scale <= 1`` raise ValueError here.

With PAB off the pair of model calls of a step is recorded once (program.Recorder) and replayed on the later steps;
``transformer.use_programs = False`` forces eager issue (the switch of the other models); with PAB on the steps run eager.

More than one rank (:266-280).  ``_set_parallel`` shards the transformer by frames (vchitect.py).  Every rank runs generate() with
the same seed, holds the whole latent and gets the whole prediction back (the model all-gathers it), so the sampler, the recorded
step (collectives are re-issued from the program's host actions) and the returned frames are the same on every rank; the text encoders
stay replicated.  The VAE decode is shared: rank r decodes a contiguous block of ceil(F / P) frames and one all-gather hands every rank
every frame (``_decode_group``; ``VchitectConfig(shard_vae_decode=False)`` or ``VSYS_VAE_SHARD=0``: every rank decodes every frame, as
the reference does)."""
from __future__ import annotations

import inspect
import logging
import math
import os
from typing import Any, Callable, Dict, List, Optional, Union

import numpy as np
import torch

from . import ops, pab, program
from .pab import PABConfig
from .pipeline import (VideoSysPipeline, VideoSysPipelineOutput, build_clip_encoder, build_text_encoder, is_foreign_module,
                       module_state)
from .utils import ctor_kwargs, progress_wrap, randn_tensor as _randn, read_component
from .clip import CLIP_BIGG, CLIP_L, CLIPTextEncoder
from .vchitect import VchitectXLTransformerModel, synth_state_dict


class VchitectPABConfig(PABConfig):
    """pipeline_vchitect.py:32-55 — identical defaults."""

    def __init__(self, spatial_broadcast: bool = True, spatial_threshold: list = [100, 800], spatial_range: int = 2,
                 temporal_broadcast: bool = True, temporal_threshold: list = [100, 800], temporal_range: int = 4,
                 cross_broadcast: bool = True, cross_threshold: list = [100, 800], cross_range: int = 6):
        super().__init__(
            spatial_broadcast=spatial_broadcast, spatial_threshold=spatial_threshold, spatial_range=spatial_range,
            temporal_broadcast=temporal_broadcast, temporal_threshold=temporal_threshold, temporal_range=temporal_range,
            cross_broadcast=cross_broadcast, cross_threshold=cross_threshold, cross_range=cross_range,
        )


class VchitectConfig:
    """pipeline_vchitect.py:58-123 — identical kwargs / defaults.  ``model_path``: a LOCAL checkpoint directory in the published layout,
    ``"synthetic:<seed>"`` (seeded transformer and SD3 VAE weights, the spelling of LatteConfig), or a hub id (cannot be fetched here: the
    published geometry with seeded transformer weights, no VAE)."""

    def __init__(self, model_path: str = "Vchitect/Vchitect-2.0-2B", num_gpus: int = 1, cpu_offload: bool = False,
                 enable_pab: bool = False, pab_config: VchitectPABConfig = VchitectPABConfig(), **extra):
        self.model_path = model_path
        self.pipeline_cls = VchitectXLPipeline
        self.num_gpus = num_gpus
        self.cpu_offload = cpu_offload
        self.enable_pab = enable_pab
        self.pab_config = pab_config
        self.transformer_config = extra.pop("transformer_config", None)  # extension: geometry override for tests
        # extension: geometry overrides of the two "synthetic:<seed>" CLIP encoders, {"text_encoder": {...}, "text_encoder_2": {...}}
        self.clip_config = extra.pop("clip_config", None)
        # extension: with num_gpus > 1 the frames of the VAE decode are sharded over the ranks and gathered once (the reference decodes
        # every frame on every rank: pipeline_vchitect.py:980-985 under engine.py:85-95); False = the reference's behaviour
        self.shard_vae_decode = bool(extra.pop("shard_vae_decode", True))
        if extra:
            raise TypeError(f"unexpected VchitectConfig kwargs: {sorted(extra)}")


class FlowMatchEulerDiscreteScheduler:
    """diffusers FlowMatchEulerDiscreteScheduler as pipeline_vchitect.py:223,895-897,952 uses it.  UNPINNED restatement: diffusers is
    third-party, not vendored by the reference and not installed here, so no fixture of the class backs this one; it is held to the
    closed form below (tests/test_vchitect_pipeline_cpu.py).

      __init__        t = linspace(1, N, N)[::-1] (fp32), s = t / N, s = shift s / (1 + (shift - 1) s); sigma_max = s[0], sigma_min = s[-1]
      set_timesteps   t = linspace(sigma_max N, sigma_min N, n), s = t / N, the shift formula AGAIN; timesteps = s N (fp32),
                      sigmas = cat(s, [0]).  It takes no ``timesteps=``: retrieve_timesteps raises for a custom schedule.
      step            prev = float32(sample) + (sigma_next - sigma) * model_output; the step index advances by one."""

    order = 1
    init_noise_sigma = 1.0

    def __init__(self, num_train_timesteps: int = 1000, shift: float = 1.0):
        self.num_train_timesteps, self.shift = num_train_timesteps, shift
        N = num_train_timesteps
        t = np.linspace(1, N, N, dtype=np.float32)[::-1].copy()
        s = t / np.float32(N)
        s = (shift * s / (1 + (shift - 1) * s)).astype(np.float32)
        self.sigma_max, self.sigma_min = float(s[0]), float(s[-1])
        self.timesteps = torch.from_numpy(s * np.float32(N))
        self.sigmas = torch.from_numpy(s)
        self.num_inference_steps = None
        self._step_index = None

    step_index = property(lambda self: self._step_index)

    def set_timesteps(self, num_inference_steps: int, device=None):
        self.num_inference_steps = num_inference_steps
        N, shift = self.num_train_timesteps, self.shift
        t = np.linspace(self.sigma_max * N, self.sigma_min * N, num_inference_steps)
        s = t / N
        s = torch.from_numpy(shift * s / (1 + (shift - 1) * s)).to(torch.float32)
        self.timesteps = s * N
        self.sigmas = torch.cat([s, torch.zeros(1, dtype=torch.float32)])
        self._step_index = None

    def step_dt(self, i: int) -> float:
        """sigma_next - sigma of step ``i`` (the fp32 difference the reference's step multiplies the prediction by)."""
        return float(self.sigmas[i + 1] - self.sigmas[i])

    def step(self, model_output, timestep, sample, return_dict: bool = True):
        if self._step_index is None:
            self._step_index = 0
        i = self._step_index
        prev = sample.to(torch.float32) + (self.sigmas[i + 1] - self.sigmas[i]).to(sample.device) * model_output
        self._step_index = i + 1
        return (prev,)


def retrieve_timesteps(scheduler, num_inference_steps: Optional[int] = None, device=None, timesteps: Optional[List[int]] = None,
                       sigmas: Optional[List[float]] = None, **kwargs):
    """pipeline_vchitect.py:1001-1057 (the diffusers helper): custom ``timesteps`` / ``sigmas`` only for schedulers whose
    ``set_timesteps`` takes them — the flow-match scheduler does not, so both raise ValueError."""
    if timesteps is not None and sigmas is not None:
        raise ValueError("Only one of `timesteps` or `sigmas` can be passed. Please choose one to set custom values")
    if timesteps is not None:
        if "timesteps" not in set(inspect.signature(scheduler.set_timesteps).parameters.keys()):
            raise ValueError(f"The current scheduler class {scheduler.__class__}'s `set_timesteps` does not support custom"
                             f" timestep schedules. Please check whether you are using the correct scheduler.")
        scheduler.set_timesteps(timesteps=timesteps, device=device, **kwargs)
        timesteps = scheduler.timesteps
        num_inference_steps = len(timesteps)
    elif sigmas is not None:
        if "sigmas" not in set(inspect.signature(scheduler.set_timesteps).parameters.keys()):
            raise ValueError(f"The current scheduler class {scheduler.__class__}'s `set_timesteps` does not support custom"
                             f" sigmas schedules. Please check whether you are using the correct scheduler.")
        scheduler.set_timesteps(sigmas=sigmas, device=device, **kwargs)
        timesteps = scheduler.timesteps
        num_inference_steps = len(timesteps)
    else:
        scheduler.set_timesteps(num_inference_steps, device=device, **kwargs)
        timesteps = scheduler.timesteps
    return timesteps, num_inference_steps


def guidance_at(guidance_scale: float, num_inference_steps: int, t: float) -> float:
    """The per-step guidance scale of :942-944 in Python doubles (the base is negative for t > N; the exponent 5.0 keeps it real)."""
    return 1 + guidance_scale * ((1 - math.cos(math.pi * ((num_inference_steps - t) / num_inference_steps) ** 5.0)) / 2)


class VchitectXLPipeline(VideoSysPipeline):
    model_cpu_offload_seq = "text_encoder->text_encoder_2->text_encoder_3->transformer->vae"
    _optional_components = ["text_encoder", "text_encoder_2", "text_encoder_3", "tokenizer", "tokenizer_2", "tokenizer_3", "vae",
                            "transformer", "scheduler"]
    _callback_tensor_inputs = ["latents", "prompt_embeds", "negative_prompt_embeds", "negative_pooled_prompt_embeds"]
    _guidance_scale, _clip_skip, _joint_attention_kwargs, _num_timesteps, _interrupt = None, None, None, 0, False

    def __init__(self, config: VchitectConfig, text_encoder=None, text_encoder_2=None, text_encoder_3=None, tokenizer=None,
                 tokenizer_2=None, tokenizer_3=None, vae=None, transformer=None, scheduler=None,
                 device: torch.device = torch.device("cuda"), dtype: torch.dtype = torch.bfloat16):
        """pipeline_vchitect.py:174-264, same parameter order.  Components left at None are read from ``config.model_path`` when that is
        a LOCAL checkpoint directory in the published layout (``transformer/``, ``vae/``, ``scheduler/``, ``text_encoder_3/`` +
        ``tokenizer_3/``); ``"synthetic:<seed>"`` builds seeded transformer and SD3 VAE weights; a hub id cannot be fetched (published
        geometry, seeded transformer weights, no VAE: generate() then returns latents).  ``text_encoder`` / ``text_encoder_2``:
        ``"synthetic:<seed>"``, a directory, a torch module with the HF weights, an injected CLIP object, or None = ``text_encoder/`` /
        ``text_encoder_2/`` (+ ``tokenizer/`` / ``tokenizer_2/``) of a local ``model_path`` (pipeline.build_clip_encoder).  ``text_encoder_3``: a t5.T5TextEncoder-like callable, a torch module holding HF T5
        weights (+ ``tokenizer_3``), a directory or ``"synthetic:<seed>"`` (pipeline.build_text_encoder); None = the zeros of :295-300."""
        self._config = config
        self._dtype = self._check_dtype(dtype)
        self._device = self._resolve_device(device, "VchitectXLPipeline")
        name = config.model_path
        synthetic = isinstance(name, str) and name.startswith("synthetic:")
        seed = int(name.split(":", 1)[1]) if synthetic else 4321
        if transformer is None or is_foreign_module(transformer, VchitectXLTransformerModel):
            file_cfg, sd = module_state(transformer) if transformer is not None else read_component(name, "transformer")
            tcfg = ctor_kwargs(VchitectXLTransformerModel.__init__, file_cfg)
            tcfg.update(config.transformer_config or {})
            transformer = VchitectXLTransformerModel(**tcfg, device=self._device)
            if sd is None:
                c = transformer.config
                sd = synth_state_dict(c.num_layers, c.num_attention_heads, c.in_channels, c.out_channels, c.patch_size,
                                      c.joint_attention_dim, c.pooled_projection_dim, seed=seed)
            transformer.load_state_dict(sd)
        self.transformer = transformer
        if scheduler is None:   # <model_path>/scheduler/scheduler_config.json (:222-223)
            scheduler = FlowMatchEulerDiscreteScheduler(**ctor_kwargs(FlowMatchEulerDiscreteScheduler.__init__,
                                                                      read_component(name, "scheduler")[0]))
        self.scheduler = self._check_scheduler(scheduler, "step_dt", "videosys_amd.pipeline_vchitect.FlowMatchEulerDiscreteScheduler")
        if vae is None:
            vae = self._load_vae(name, seed if synthetic else None)
        elif is_foreign_module(vae):
            vae = self._vae_from_state(*module_state(vae))
        self.vae = vae
        clips = []
        for sub, tok_sub, spec, tok in (("text_encoder", "tokenizer", text_encoder, tokenizer),
                                        ("text_encoder_2", "tokenizer_2", text_encoder_2, tokenizer_2)):
            tok_path = None
            if spec is None and isinstance(name, str) and os.path.isdir(os.path.join(name, sub)):   # (:194-201 from_pretrained subfolders)
                spec, tok_path = os.path.join(name, sub), os.path.join(name, tok_sub)
            clips.append(build_clip_encoder(spec, tok, device=self._device, geometry=self._clip_geometry(sub), tokenizer_path=tok_path))
        (self.text_encoder, self.tokenizer), (self.text_encoder_2, self.tokenizer_2) = clips
        widths = [e.config.hidden_size for e in (self.text_encoder, self.text_encoder_2) if isinstance(e, CLIPTextEncoder)]
        if sum(widths) > self.transformer.config.joint_attention_dim:
            raise ValueError(f"the CLIP hidden sizes {widths} side by side are wider than joint_attention_dim = "
                             f"{self.transformer.config.joint_attention_dim}: encode_prompt pads them to the T5 width (:494-496)")
        if text_encoder_3 is None and isinstance(name, str) and os.path.isdir(os.path.join(name, "text_encoder_3")):
            text_encoder_3 = os.path.join(name, "text_encoder_3")
        self.max_sequence_length_t5 = 256
        # the reference hands T5 no attention mask (:320): the padding is attended
        self.text_encoder_3 = build_text_encoder(text_encoder_3, tokenizer_3, device=self._device,
                                                 caption_channels=self.transformer.config.joint_attention_dim,
                                                 max_length=self.max_sequence_length_t5, use_attention_mask=False,
                                                 tokenizer_path=os.path.join(name, "tokenizer_3") if isinstance(name, str) else None)
        pab.set_pab_manager(config.pab_config if config.enable_pab else None)
        self.vae_scale_factor = 2 ** (len(self.vae.config.block_out_channels) - 1) if self.vae is not None else 8
        self.tokenizer_max_length = getattr(self.tokenizer, "model_max_length", 77) if self.tokenizer is not None else 77
        self.default_sample_size = self.transformer.config.sample_size
        self._steps = program.StepCache()   # (latent shape, text shape) -> (Program, (z, enc, pooled, pred)): one entry at a time
        self.pab_trace: List[list] = []   # PAB on: per model call of the last generate(), every block's (temporal, cross, spatial)
        self._set_parallel()
        own_clip = lambda e: e if isinstance(e, CLIPTextEncoder) else None   # (injected objects look after their own weights)
        self._init_stages(config.cpu_offload, self._device, text_encoder=own_clip(self.text_encoder),
                          text_encoder_2=own_clip(self.text_encoder_2), text_encoder_3=getattr(self.text_encoder_3, "encoder", None),
                          transformer=self.transformer, vae=self.vae)

    tokenizer_3 = property(lambda self: getattr(self.text_encoder_3, "tokenizer", None))
    vae_decoder = property(lambda self: self.vae)
    step_stats = program.stats_property("_steps")

    def _clip_geometry(self, slot: str) -> dict:
        """Constructor keywords of the ``"synthetic:<seed>"`` encoder of ``slot``: CLIP-L for ``text_encoder``, CLIP-bigG for
        ``text_encoder_2``.  The transformer's ``pooled_projection_dim`` is the two ``projection_dim``s side by side, split 3 : 5
        (2048 = 768 + 1280); ``config.clip_config[slot]`` overrides single fields."""
        pd = self.transformer.config.pooled_projection_dim
        first = pd * 3 // 8
        geo = dict(CLIP_L, projection_dim=first) if slot == "text_encoder" else dict(CLIP_BIGG, projection_dim=pd - first)
        geo.update((getattr(self._config, "clip_config", None) or {}).get(slot, {}))
        return geo

    def _vae_from_state(self, cfg, sd):
        from .vae_sd3 import SCALING_FACTOR, SHIFT_FACTOR, AutoencoderKLSD3Decoder

        return AutoencoderKLSD3Decoder(sd, device=self._device, scaling_factor=cfg.get("scaling_factor", SCALING_FACTOR),
                                       shift_factor=cfg.get("shift_factor", SHIFT_FACTOR))

    def _load_vae(self, name, synthetic_seed):
        """:214-215 AutoencoderKL.from_pretrained(model_path, subfolder="vae"): local ``diffusion_pytorch_model.safetensors`` +
        config.json, or seeded weights for ``"synthetic:<seed>"``; None when neither is there."""
        from .vae_sd3 import AutoencoderKLSD3Decoder, synth_state_dict as vae_synth

        if synthetic_seed is not None:
            return AutoencoderKLSD3Decoder(vae_synth(synthetic_seed), device=self._device)
        if not isinstance(name, str):
            return None
        cfg, sd = read_component(name, "vae")
        return self._vae_from_state(cfg, sd) if sd is not None else None

    def _set_parallel(self, dp_size: Optional[int] = None, sp_size: Optional[int] = None, enable_cp: Optional[bool] = False,
                      parallel_mgr=None):
        """pipeline_vchitect.py:266-280: sp = world size unless given.  The transformer is sharded by frames (vchitect.py: every rank
        calls generate() with the same seed and gets the same frames, the model gathering its prediction inside); the text encoders
        stay replicated, the VAE decode is shared over the same group by frames (``_decode_group``).  ``parallel_mgr`` (an
        extension): an injected manager instead of the process group, as the transformers take it."""
        self._steps.clear()                # a recorded step belongs to the sharding it was recorded under
        if parallel_mgr is not None:
            return self.transformer.enable_parallel(parallel_mgr=parallel_mgr)
        if self._world_size() > 1:
            self.transformer.enable_parallel(*self._parallel_sizes(sp_size), enable_cp)

    # ------------------------------------------------------------------------------------------------ text side
    def _get_t5_prompt_embeds(self, prompt: Union[str, List[str]] = None, num_images_per_prompt: int = 1, device=None, dtype=None):
        """pipeline_vchitect.py:282-331 -> [B * num_images_per_prompt, 256, joint_attention_dim]; zeros without ``text_encoder_3``."""
        device = device or self._device
        prompt = [prompt] if isinstance(prompt, str) else prompt
        batch_size = len(prompt)
        if self.text_encoder_3 is None:
            return torch.zeros((batch_size, self.max_sequence_length_t5, self.transformer.config.joint_attention_dim), device=device,
                               dtype=dtype or self._dtype)
        self._enter_stage("text_encoder_3")
        e = self.text_encoder_3(list(prompt))
        e = e[0] if isinstance(e, tuple) else e
        e = e.reshape(batch_size, e.shape[-2], e.shape[-1]).to(device=device)
        _, seq_len, _ = e.shape
        return e.repeat(1, num_images_per_prompt, 1).view(batch_size * num_images_per_prompt, seq_len, -1)

    def _get_clip_prompt_embeds(self, prompt: Union[str, List[str]], num_images_per_prompt: int = 1, device=None,
                                clip_skip: Optional[int] = None, clip_model_index: int = 0):
        """pipeline_vchitect.py:333-386 on the CLIP encoder of the slot -> (prompt_embeds [B, 77, d], pooled [B, d'])."""
        device = device or self._device
        tokenizer = [self.tokenizer, self.tokenizer_2][clip_model_index]
        text_encoder = [self.text_encoder, self.text_encoder_2][clip_model_index]
        if text_encoder is None or tokenizer is None:
            raise RuntimeError(self._NO_CLIP)
        prompt = [prompt] if isinstance(prompt, str) else prompt
        batch_size = len(prompt)
        text_input_ids = tokenizer(prompt, padding="max_length", max_length=self.tokenizer_max_length, truncation=True,
                                   return_tensors="pt").input_ids
        untruncated_ids = tokenizer(prompt, padding="longest", return_tensors="pt").input_ids
        if untruncated_ids.shape[-1] >= text_input_ids.shape[-1] and not torch.equal(text_input_ids, untruncated_ids):
            removed_text = tokenizer.batch_decode(untruncated_ids[:, self.tokenizer_max_length - 1: -1])
            logging.warning("The following part of your input was truncated because CLIP can only handle sequences up to"
                            f" {self.tokenizer_max_length} tokens: {removed_text}")
        self._enter_stage(("text_encoder", "text_encoder_2")[clip_model_index])   # (cpu_offload: model_cpu_offload_seq order)
        prompt_embeds = text_encoder(text_input_ids.to(device), output_hidden_states=True)
        pooled_prompt_embeds = prompt_embeds[0]
        if clip_skip is None:
            prompt_embeds = prompt_embeds.hidden_states[-2]
        else:
            prompt_embeds = prompt_embeds.hidden_states[-(clip_skip + 2)]
        prompt_embeds = prompt_embeds.to(dtype=self._dtype, device=device)
        _, seq_len, _ = prompt_embeds.shape
        prompt_embeds = prompt_embeds.repeat(1, num_images_per_prompt, 1).view(batch_size * num_images_per_prompt, seq_len, -1)
        pooled_prompt_embeds = pooled_prompt_embeds.repeat(1, num_images_per_prompt, 1).view(batch_size * num_images_per_prompt, -1)
        return prompt_embeds, pooled_prompt_embeds

    _NO_CLIP = ("the CLIP encoders of Vchitect-2.0 (CLIP-L, CLIP-bigG) are not built in this package: either construct the pipeline "
                "with text_encoder= / text_encoder_2= objects (and tokenizer= / tokenizer_2=) that are called as "
                "CLIPTextModelWithProjection is, or pass prompt_embeds + pooled_prompt_embeds and negative_prompt_embeds + "
                "negative_pooled_prompt_embeds to generate()")

    def encode_prompt(self, prompt, prompt_2, prompt_3, device=None, num_images_per_prompt: int = 1,
                      do_classifier_free_guidance: bool = True, negative_prompt=None, negative_prompt_2=None, negative_prompt_3=None,
                      prompt_embeds: Optional[torch.Tensor] = None, negative_prompt_embeds: Optional[torch.Tensor] = None,
                      pooled_prompt_embeds: Optional[torch.Tensor] = None, negative_pooled_prompt_embeds: Optional[torch.Tensor] = None,
                      clip_skip: Optional[int] = None):
        """pipeline_vchitect.py:395-562 -> (prompt_embeds [B, 77 + 256, D], negative_prompt_embeds, pooled [B, 2048], negative pooled):
        [CLIP-L | CLIP-bigG] hidden states zero-padded to the T5 width, then the T5 states."""
        device = device or self._device
        prompt = [prompt] if isinstance(prompt, str) else prompt
        batch_size = len(prompt) if prompt is not None else prompt_embeds.shape[0]
        if prompt_embeds is None:
            prompt_2 = prompt_2 or prompt
            prompt_2 = [prompt_2] if isinstance(prompt_2, str) else prompt_2
            prompt_3 = prompt_3 or prompt
            prompt_3 = [prompt_3] if isinstance(prompt_3, str) else prompt_3
            prompt_embed, pooled_prompt_embed = self._get_clip_prompt_embeds(prompt, num_images_per_prompt, device, clip_skip, 0)
            prompt_2_embed, pooled_prompt_2_embed = self._get_clip_prompt_embeds(prompt_2, num_images_per_prompt, device, clip_skip, 1)
            clip_prompt_embeds = torch.cat([prompt_embed, prompt_2_embed], dim=-1)
            t5_prompt_embed = self._get_t5_prompt_embeds(prompt_3, num_images_per_prompt, device).to(clip_prompt_embeds.dtype)
            clip_prompt_embeds = torch.nn.functional.pad(clip_prompt_embeds, (0, t5_prompt_embed.shape[-1] - clip_prompt_embeds.shape[-1]))
            prompt_embeds = torch.cat([clip_prompt_embeds, t5_prompt_embed], dim=-2)
            pooled_prompt_embeds = torch.cat([pooled_prompt_embed, pooled_prompt_2_embed], dim=-1)
        if do_classifier_free_guidance and negative_prompt_embeds is None:
            negative_prompt = negative_prompt or ""
            negative_prompt_2 = negative_prompt_2 or negative_prompt
            negative_prompt_3 = negative_prompt_3 or negative_prompt
            negative_prompt = batch_size * [negative_prompt] if isinstance(negative_prompt, str) else negative_prompt
            negative_prompt_2 = batch_size * [negative_prompt_2] if isinstance(negative_prompt_2, str) else negative_prompt_2
            negative_prompt_3 = batch_size * [negative_prompt_3] if isinstance(negative_prompt_3, str) else negative_prompt_3
            if prompt is not None and type(prompt) is not type(negative_prompt):
                raise TypeError(f"`negative_prompt` should be the same type to `prompt`, but got {type(negative_prompt)} !="
                                f" {type(prompt)}.")
            elif batch_size != len(negative_prompt):
                raise ValueError(f"`negative_prompt`: {negative_prompt} has batch size {len(negative_prompt)}, but `prompt`:"
                                 f" {prompt} has batch size {batch_size}. Please make sure that passed `negative_prompt` matches"
                                 " the batch size of `prompt`.")
            ne, npe = self._get_clip_prompt_embeds(negative_prompt, num_images_per_prompt, device, None, 0)
            ne2, npe2 = self._get_clip_prompt_embeds(negative_prompt_2, num_images_per_prompt, device, None, 1)
            negative_clip = torch.cat([ne, ne2], dim=-1)
            t5_neg = self._get_t5_prompt_embeds(negative_prompt_3, num_images_per_prompt, device).to(negative_clip.dtype)
            negative_clip = torch.nn.functional.pad(negative_clip, (0, t5_neg.shape[-1] - negative_clip.shape[-1]))
            negative_prompt_embeds = torch.cat([negative_clip, t5_neg], dim=-2)
            negative_pooled_prompt_embeds = torch.cat([npe, npe2], dim=-1)
        to = lambda t: None if t is None else t.to(self._device)
        return to(prompt_embeds), to(negative_prompt_embeds), to(pooled_prompt_embeds), to(negative_pooled_prompt_embeds)

    def check_inputs(self, prompt, prompt_2, prompt_3, height, width, negative_prompt=None, negative_prompt_2=None,
                     negative_prompt_3=None, prompt_embeds=None, negative_prompt_embeds=None, pooled_prompt_embeds=None,
                     negative_pooled_prompt_embeds=None, callback_on_step_end_tensor_inputs=None):
        """pipeline_vchitect.py:564-648: the argument combinations the reference refuses, with its ValueErrors."""
        if height % 8 != 0 or width % 8 != 0:
            raise ValueError(f"`height` and `width` have to be divisible by 8 but are {height} and {width}.")
        if callback_on_step_end_tensor_inputs is not None and not all(k in self._callback_tensor_inputs for k in callback_on_step_end_tensor_inputs):
            raise ValueError(f"`callback_on_step_end_tensor_inputs` has to be in {self._callback_tensor_inputs}, but found "
                             f"{[k for k in callback_on_step_end_tensor_inputs if k not in self._callback_tensor_inputs]}")
        both = "Please make sure to only forward one of the two."
        if prompt is not None and prompt_embeds is not None:
            raise ValueError(f"Cannot forward both `prompt`: {prompt} and `prompt_embeds`. {both}")
        elif prompt_2 is not None and prompt_embeds is not None:
            raise ValueError(f"Cannot forward both `prompt_2`: {prompt_2} and `prompt_embeds`. {both}")
        elif prompt_3 is not None and prompt_embeds is not None:
            raise ValueError(f"Cannot forward both `prompt_3`: {prompt_3} and `prompt_embeds`. {both}")
        elif prompt is None and prompt_embeds is None:
            raise ValueError("Provide either `prompt` or `prompt_embeds`. Cannot leave both `prompt` and `prompt_embeds` undefined.")
        elif prompt is not None and (not isinstance(prompt, str) and not isinstance(prompt, list)):
            raise ValueError(f"`prompt` has to be of type `str` or `list` but is {type(prompt)}")
        elif prompt_2 is not None and (not isinstance(prompt_2, str) and not isinstance(prompt_2, list)):
            raise ValueError(f"`prompt_2` has to be of type `str` or `list` but is {type(prompt_2)}")
        elif prompt_3 is not None and (not isinstance(prompt_3, str) and not isinstance(prompt_3, list)):
            raise ValueError(f"`prompt_3` has to be of type `str` or `list` but is {type(prompt_3)}")
        if negative_prompt is not None and negative_prompt_embeds is not None:
            raise ValueError(f"Cannot forward both `negative_prompt`: {negative_prompt} and `negative_prompt_embeds`. {both}")
        elif negative_prompt_2 is not None and negative_prompt_embeds is not None:
            raise ValueError(f"Cannot forward both `negative_prompt_2`: {negative_prompt_2} and `negative_prompt_embeds`. {both}")
        elif negative_prompt_3 is not None and negative_prompt_embeds is not None:
            raise ValueError(f"Cannot forward both `negative_prompt_3`: {negative_prompt_3} and `negative_prompt_embeds`. {both}")
        if prompt_embeds is not None and negative_prompt_embeds is not None:
            if prompt_embeds.shape != negative_prompt_embeds.shape:
                raise ValueError("`prompt_embeds` and `negative_prompt_embeds` must have the same shape when passed directly, but"
                                 f" got: `prompt_embeds` {prompt_embeds.shape} != `negative_prompt_embeds` {negative_prompt_embeds.shape}.")
        if prompt_embeds is not None and pooled_prompt_embeds is None:
            raise ValueError("If `prompt_embeds` are provided, `pooled_prompt_embeds` also have to be passed. Make sure to generate "
                             "`pooled_prompt_embeds` from the same text encoder that was used to generate `prompt_embeds`.")
        if negative_prompt_embeds is not None and negative_pooled_prompt_embeds is None:
            raise ValueError("If `negative_prompt_embeds` are provided, `negative_pooled_prompt_embeds` also have to be passed. Make sure "
                             "to generate `negative_pooled_prompt_embeds` from the same text encoder that was used to generate "
                             "`negative_prompt_embeds`.")

    def prepare_latents(self, batch_size, num_channels_latents, height, width, frames, dtype, device, generator, latents=None):
        """pipeline_vchitect.py:650-681: start latents [B, F, C, h / 8, w / 8] drawn from ``generator`` (utils.randn_tensor) unless
        handed in."""
        if latents is not None:
            return latents.to(device=device, dtype=dtype)
        shape = (batch_size, frames, num_channels_latents, int(height) // self.vae_scale_factor, int(width) // self.vae_scale_factor)
        if isinstance(generator, list) and len(generator) != batch_size:
            raise ValueError(f"You have passed a list of generators of length {len(generator)}, but requested an effective batch"
                             f" size of {batch_size}. Make sure the batch size matches the length of the generators.")
        return _randn(shape, generator, dtype).to(device=device, dtype=dtype)

    guidance_scale = property(lambda self: self._guidance_scale)                    # (:683-708)
    clip_skip = property(lambda self: self._clip_skip)
    do_classifier_free_guidance = property(lambda self: self._guidance_scale > 1)
    joint_attention_kwargs = property(lambda self: self._joint_attention_kwargs)
    num_timesteps = property(lambda self: self._num_timesteps)
    interrupt = property(lambda self: self._interrupt)

    # ------------------------------------------------------------------------------------------------ denoise step
    def _model_pair(self, z, enc, pooled, pred, t):
        """The two model calls of a step in the reference's order (:925-941): uncond (row 0 of the CFG pair) into pred[1], text (row 1)
        into pred[0].  ``enc`` [2, F, L, D] / ``pooled`` [2, PD]: (negative, prompt)."""
        ts = torch.tensor([float(t)])
        for row, dst in ((0, 1), (1, 0)):
            self.transformer(z, encoder_hidden_states=enc[row], pooled_projections=pooled[row:row + 1], timestep=ts,
                             joint_attention_kwargs=self._joint_attention_kwargs, return_dict=False, out=pred[dst])
            if pab.enable_pab():
                self.pab_trace.append([blk.attn.last_decisions for blk in self.transformer.transformer_blocks])

    def _issue_pair(self, z, enc, pooled, pred, t):
        """_model_pair eagerly (PAB on, ``transformer.use_programs`` False, or something unrecordable ran), else through the launch
        program recorded at the first step of this (geometry, embeddings)."""
        tr = self.transformer
        if pab.enable_pab() or not getattr(tr, "use_programs", True):
            return self._steps.eager(lambda: self._model_pair(z, enc, pooled, pred, t))

        def record():
            self._model_pair(z, enc, pooled, pred, t)
            return z, enc, pooled, pred

        # (on a hit) the one per-step input besides the latents, updated in place
        self._steps.run(self._step_key(z, enc), record, lambda bufs: tr.step_timesteps(z.shape[1]).fill_(float(t)))

    @staticmethod
    def _step_key(z, enc):
        return tuple(z.shape), tuple(enc.shape)

    def _step_buffers(self, z0, prompt_embeds, pooled):
        """Resident inputs of a step: latents z fp32 [1, F, 16, h, w], enc bf16 [2, F, L, D] (every frame reads its sample's prompt),
        pooled bf16 [2, PD], pred fp32 [2, F, 16, h, w].  A recorded program holds their addresses: the buffers of the last generate()
        are reused (and the program with them) when geometry and embeddings are the same, else new ones are made and the program is
        dropped, so that a key of the cache never names buffers other than the ones in use."""
        F = z0.shape[1]
        enc = prompt_embeds.to(device=self._device, dtype=torch.bfloat16)[:, None].expand(2, F, *prompt_embeds.shape[1:]).contiguous()
        pooled = pooled.to(device=self._device, dtype=torch.bfloat16).contiguous()
        ent = self._steps.entries.get(self._step_key(z0, enc))
        if ent is not None and torch.equal(ent[1][1], enc) and torch.equal(ent[1][2], pooled):
            ent[1][0].copy_(z0)
            return ent[1]
        self._steps.clear()
        z = z0.to(device=self._device, dtype=torch.float32).contiguous().clone()
        return z, enc, pooled, torch.empty((2,) + tuple(z.shape[1:]), dtype=torch.float32, device=self._device)

    @torch.no_grad()
    def generate(self, prompt: Union[str, List[str]] = None, prompt_2: Optional[Union[str, List[str]]] = None,
                 prompt_3: Optional[Union[str, List[str]]] = None, height: int = 288, width: int = 480, frames: int = 40,
                 num_inference_steps: int = 100, timesteps: List[int] = None, guidance_scale: float = 7.5, seed: int = -1,
                 negative_prompt: Optional[Union[str, List[str]]] = None, negative_prompt_2: Optional[Union[str, List[str]]] = None,
                 negative_prompt_3: Optional[Union[str, List[str]]] = None, num_images_per_prompt: Optional[int] = 1,
                 generator: Optional[Union[torch.Generator, List[torch.Generator]]] = None, latents: Optional[torch.FloatTensor] = None,
                 prompt_embeds: Optional[torch.FloatTensor] = None, negative_prompt_embeds: Optional[torch.FloatTensor] = None,
                 pooled_prompt_embeds: Optional[torch.FloatTensor] = None,
                 negative_pooled_prompt_embeds: Optional[torch.FloatTensor] = None, output_type: Optional[str] = "pil",
                 return_dict: bool = True, joint_attention_kwargs: Optional[Dict[str, Any]] = None, clip_skip: Optional[int] = None,
                 callback_on_step_end: Optional[Callable[[int, int, Dict], None]] = None,
                 callback_on_step_end_tensor_inputs: List[str] = ["latents"]):
        """pipeline_vchitect.py:712-994 with the reference's parameters and defaults (module docstring for the sampler, the batch
        rules and the guidance corner).  ``output_type``: "pil" (a list of F PIL images), "np" (float arrays in [0, 1], as
        VaeImageProcessor.postprocess), "pt" (the same as a tensor [F, 3, H, W]) or "latent" (the fp32 latents; also what comes back
        when no VAE is attached).  ``callback_on_step_end(self, i, t, {...})`` sees the tensors named in
        ``callback_on_step_end_tensor_inputs`` and may hand back new ones; setting ``pipe._interrupt`` skips the remaining steps.
        Returns ``VideoSysPipelineOutput(video=[frames])``."""
        height = height or self.default_sample_size * self.vae_scale_factor
        width = width or self.default_sample_size * self.vae_scale_factor
        frames = frames or 24
        seed = self._set_seed(seed)
        pab.update_steps(num_inference_steps)
        self.check_inputs(prompt, prompt_2, prompt_3, height, width, negative_prompt=negative_prompt,
                          negative_prompt_2=negative_prompt_2, negative_prompt_3=negative_prompt_3, prompt_embeds=prompt_embeds,
                          negative_prompt_embeds=negative_prompt_embeds, pooled_prompt_embeds=pooled_prompt_embeds,
                          negative_pooled_prompt_embeds=negative_pooled_prompt_embeds,
                          callback_on_step_end_tensor_inputs=callback_on_step_end_tensor_inputs)
        if isinstance(prompt, list) and len(prompt) != 1:
            raise ValueError(f"Vchitect generates one prompt per call: the reference's loop reads rows 0 and 1 of the guidance pair "
                             f"(pipeline_vchitect.py:925-941); got a list of {len(prompt)} prompts")
        if prompt_embeds is not None and prompt_embeds.shape[0] != 1:
            raise ValueError(f"Vchitect generates one prompt per call; got prompt_embeds for {prompt_embeds.shape[0]}")
        if num_images_per_prompt != 1:
            raise ValueError(f"num_images_per_prompt must be 1 (the reference's loop reads rows 0 and 1 of the guidance pair); got {num_images_per_prompt}")
        if not guidance_scale > 1:
            raise ValueError(f"guidance_scale must be above 1: without classifier-free guidance the reference's loop has no second row to "
                             f"read (pipeline_vchitect.py:934-941); got {guidance_scale}")
        self._guidance_scale, self._clip_skip = guidance_scale, clip_skip
        self._joint_attention_kwargs, self._interrupt = joint_attention_kwargs, False
        have_clip = self.text_encoder is not None and self.text_encoder_2 is not None
        if not have_clip and (prompt_embeds is None or negative_prompt_embeds is None):
            raise RuntimeError(self._NO_CLIP)
        # (cpu_offload: every encoder enters its own stage when encode_prompt calls it)
        prompt_embeds, negative_prompt_embeds, pooled_prompt_embeds, negative_pooled_prompt_embeds = self.encode_prompt(
            prompt=prompt, prompt_2=prompt_2, prompt_3=prompt_3, negative_prompt=negative_prompt, negative_prompt_2=negative_prompt_2,
            negative_prompt_3=negative_prompt_3, do_classifier_free_guidance=True, prompt_embeds=prompt_embeds,
            negative_prompt_embeds=negative_prompt_embeds, pooled_prompt_embeds=pooled_prompt_embeds,
            negative_pooled_prompt_embeds=negative_pooled_prompt_embeds, device=self._device, clip_skip=clip_skip,
            num_images_per_prompt=num_images_per_prompt)
        cfg_embeds = torch.cat([negative_prompt_embeds, prompt_embeds], dim=0)                    # (:890-892)
        cfg_pooled = torch.cat([negative_pooled_prompt_embeds, pooled_prompt_embeds], dim=0)
        ts, num_inference_steps = retrieve_timesteps(self.scheduler, num_inference_steps, self._device, timesteps)
        self._num_timesteps = len(ts)
        self._enter_stage("transformer")
        self.transformer.reset_pab_state()
        self.pab_trace = []
        if latents is None and generator is None:
            generator = torch.Generator(device="cpu").manual_seed(seed)
        z0 = self.prepare_latents(1, self.transformer.config.in_channels, height, width, frames, torch.float32, self._device, generator,
                                  latents)
        z, enc, pooled, pred = self._step_buffers(z0, cfg_embeds, cfg_pooled)
        for i, t in progress_wrap(list(enumerate(ts.tolist())), True):
            if self._interrupt:
                continue
            self._issue_pair(z, enc, pooled, pred, t)
            self._guidance_scale = guidance_at(guidance_scale, num_inference_steps, t)
            ops.cfg_euler_step(z, pred, self._guidance_scale, self.scheduler.step_dt(i))
            if callback_on_step_end is not None:
                have = {"latents": z, "prompt_embeds": cfg_embeds, "negative_prompt_embeds": negative_prompt_embeds,
                        "negative_pooled_prompt_embeds": negative_pooled_prompt_embeds}
                back = callback_on_step_end(self, i, t, {k: have[k] for k in callback_on_step_end_tensor_inputs})
                back = back if isinstance(back, dict) else {}
                if back.get("latents") is not None and back["latents"] is not z:
                    z.copy_(back["latents"].to(z.device, z.dtype))
                if back.get("prompt_embeds") is not None and back["prompt_embeds"] is not cfg_embeds:
                    cfg_embeds = back["prompt_embeds"]
                    enc.copy_(cfg_embeds.to(enc.device, enc.dtype)[:, None].expand_as(enc))
                negative_prompt_embeds = back.get("negative_prompt_embeds", negative_prompt_embeds)
                negative_pooled_prompt_embeds = back.get("negative_pooled_prompt_embeds", negative_pooled_prompt_embeds)
        from . import dsp

        dsp.check_exchange(self.transformer)   # a timed-out peer-to-peer exchange left stale rows: raise here, not a corrupt video
        if self.vae is None or output_type in ("latent", "latents"):
            return self._leave(z.clone(), return_dict)
        self._enter_stage("vae")
        return self._leave([self.decode_frames(z, output_type)], return_dict)                    # (:980-986)

    def decode_frames(self, latents, output_type: str = "pil"):
        """pipeline_vchitect.py:980-985: `latents / scaling_factor + shift_factor`, every frame through the VAE, then
        VaeImageProcessor.postprocess — the first and the last of these inside the decoder's two own kernels for "pil".  Under
        sequence parallelism the frames are shared by the ranks (``_decode_group``) and every rank gets all of them."""
        grp = self._decode_group()
        kw = {} if grp is None else {"group": grp}               # (an injected VAE is called as the reference calls it)
        if output_type == "pil":
            from PIL import Image

            u8 = self.vae.decode_u8(latents.to(torch.float32), **kw).cpu().numpy()
            return [Image.fromarray(f) for f in u8]
        if output_type not in ("np", "pt"):
            raise ValueError(f"output_type {output_type!r}: expected 'pil', 'np', 'pt' or 'latent'")
        c = self.vae.config
        # (:980) on the bf16 latents; on the host, where a tensor / scalar is a true division as in the decoder's first kernel
        bf = lambda t: t.to(torch.bfloat16).float()
        zin = bf(bf(bf(latents[0].cpu()) / c.scaling_factor) + c.shift_factor).to(self._device)     # one rounding per step, fp32 between
        img = (self.vae.decode(zin, return_dict=False, **kw)[0] / 2 + 0.5).clamp(0, 1)                # denormalize, on the bf16 tensor
        if output_type == "pt":
            return img
        return list(img.cpu().permute(0, 2, 3, 1).float().numpy())

    def save_video(self, video, output_path):
        from .utils import save_video

        if isinstance(video, (list, tuple)):      # the PIL frames generate() returns
            video = torch.from_numpy(np.stack([np.asarray(f) for f in video]))
        return save_video(video, output_path, fps=8)   # the reference's frame rate for this pipeline (:996-997)
