"""Open-Sora-Plan v1.2 pipeline plug-in — host mirror of videosys/pipelines/open_sora_plan/pipeline_open_sora_plan.py
(OpenSoraPlanV120PABConfig :103-120, OpenSoraPlanConfig :123-225, OpenSoraPlanPipeline :228-1193, retrieve_timesteps :1197-1252):
prompt -> mT5 embeddings with their masks -> Euler-ancestral sampling with OpenSoraT2V (open_sora_plan.py) -> CausalVAE decode
(vae_open_sora_plan.py) -> uint8 video [B, T, H, W, 3].  The v1.1 pipeline (PNDM, its CausalVAE, T5 at 300 tokens) has classes of its own in
pipeline_open_sora_plan_v110.py (``OpenSoraPlanV110Config`` / ``OpenSoraPlanV110Pipeline``; ``OpenSoraPlanV110PABConfig`` is also
reachable from here, as in the reference's module); ``version="v110"`` on the classes below still raises.

``OpenSoraPlanConfig`` / ``OpenSoraPlanV120PABConfig`` take the reference's keywords with its defaults and drop into ``VideoSysEngine``.

Text side.  mT5-XXL has the geometry of T5 v1.1 XXL with a vocabulary of 250112 and the state-dict names of ``T5EncoderModel``
(``MT5EncoderModel`` subclasses it), so it is this build's t5.T5Encoder with ``vocab_size=250112`` and needs no loader of its own;
its attention takes up to 512 tokens, the pipeline's ``max_sequence_length``.  ``text_encoder`` takes ``"synthetic:<seed>"``, a local
directory, a torch module holding the HF weights (+ ``tokenizer``) or an injected callable (prompts -> (embeddings [B, 1, L, d], mask
[B, L])), as the Vchitect pipeline does; None = ``config.text_encoder`` when that is a local directory.  Synthetic runs tokenize with
``ByteTokenizer(vocab_size=250112)``.

Sampler.  ``EulerAncestralDiscreteScheduler`` below restates diffusers' class with its defaults (UNPINNED: its docstring).  One
model call per step on the CFG batch [negative | prompt] (:1109-1147), recorded once per (geometry, text shape, PAB decision
pattern) and replayed on the later steps of the same pattern; after each call ``vsys_cfg_ancestral_step`` does the guidance
combine, the drop of the learned-sigma half, the ancestral update of the fp32 latents and the ``scale_model_input`` of the NEXT step
in one launch.  The per-step noise is ``torch.randn`` from the caller's ``generator`` (on the device for a device generator; a CPU
generator draws on the host and the draw moves, as diffusers' randn_tensor does); the last step has sigma_up = 0 and draws none.
Without guidance (``guidance_scale <= 1``) the model runs on [prompt | prompt] at guidance 1: u + 1 (c - u) with u = c is c exactly.

``num_gpus`` = the size of the process group this process belongs to (one process per GPU; anything else raises): the transformer
runs Ulysses sequence parallelism over it (open_sora_plan.py), every rank replays its own recorded step and runs the sampler step on
the full gathered prediction; the text encoder is replicated.  The tiled CausalVAE decode is shared: its (sample, temporal chunk,
spatial tile) units are dealt over the ranks of the transformer's group and gathered once, then every rank stitches and converts to
uint8 (``_decode_group``; ``OpenSoraPlanConfig(shard_vae_decode=False)`` or ``VSYS_VAE_SHARD=0``: every rank decodes every tile, as
the reference does); a decode that does not tile stays replicated."""
from __future__ import annotations

import inspect
import math
import os
from typing import Callable, List, Optional, Tuple, Union

import numpy as np
import torch

from . import open_sora_plan_ops as oops
from . import dsp, pab, program
from .open_sora_plan import OpenSoraT2V, _NoGroupOfThatSize, synth_state_dict
from .pab import PABConfig
from .pipeline import VideoSysPipeline, VideoSysPipelineOutput, build_text_encoder, is_foreign_module, module_state
from .pipeline_vchitect import retrieve_timesteps  # noqa: F401  (the same diffusers helper, pipeline_open_sora_plan.py:1197-1252)
from .utils import ctor_kwargs, progress_wrap, randn_tensor as _randn, read_component

MT5_VOCAB = 250112
V120_TYPES = ("93x480p", "93x720p", "29x480p", "29x720p")


class OpenSoraPlanV120PABConfig(PABConfig):
    """pipeline_open_sora_plan.py:103-120 — identical defaults."""

    def __init__(self, spatial_broadcast: bool = True, spatial_threshold: list = [100, 850], spatial_range: int = 2,
                 cross_broadcast: bool = True, cross_threshold: list = [100, 850], cross_range: int = 6):
        super().__init__(spatial_broadcast=spatial_broadcast, spatial_threshold=spatial_threshold, spatial_range=spatial_range,
                         cross_broadcast=cross_broadcast, cross_threshold=cross_threshold, cross_range=cross_range)


class OpenSoraPlanConfig:
    """pipeline_open_sora_plan.py:123-225 — identical kwargs / defaults.  ``transformer``: a LOCAL checkpoint directory in the
    published layout (``<transformer_type>/``, ``vae/``), ``"synthetic:<seed>"`` (seeded transformer and CausalVAE weights), or a hub
    id (cannot be fetched here: the published geometry with seeded transformer weights, no VAE).  Extensions, for tests:
    ``transformer_config`` / ``vae_config`` (geometry overrides) and ``num_frames`` (instead of the one ``transformer_type`` names);
    ``shard_vae_decode`` (default True): see below."""

    def __init__(self, version: str = "v120", transformer_type: str = "29x480p", transformer: str = None, text_encoder: str = None,
                 num_gpus: int = 1, cpu_offload: bool = False, enable_tiling: bool = True, tile_overlap_factor: float = 0.25,
                 enable_pab: bool = False, pab_config: PABConfig = None, **extra):
        self.pipeline_cls = OpenSoraPlanPipeline
        assert version in ["v110", "v120"], f"Unknown Open-Sora-Plan version: {version}"
        if version == "v110":
            raise NotImplementedError("the Open-Sora-Plan v1.1 pipeline has classes of its own: OpenSoraPlanV110Config / "
                                      "OpenSoraPlanV110Pipeline (pipeline_open_sora_plan_v110.py); this class builds version='v120'")
        self.version = version
        assert transformer_type in V120_TYPES, f"transformer_type must be one of {V120_TYPES}"
        self.transformer_type = transformer_type
        self.num_frames = int(extra.pop("num_frames", None) or transformer_type.split("x")[0])
        self.text_encoder = text_encoder or "google/mt5-xxl"
        self.transformer = transformer or "LanguageBind/Open-Sora-Plan-v1.2.0"
        self.num_gpus = num_gpus
        self.cpu_offload = cpu_offload
        self.enable_tiling = enable_tiling
        self.tile_overlap_factor = tile_overlap_factor
        self.enable_pab = enable_pab
        self.pab_config = OpenSoraPlanV120PABConfig() if (enable_pab and pab_config is None) else pab_config
        self.transformer_config = extra.pop("transformer_config", None)
        self.vae_config = extra.pop("vae_config", None)
        # with num_gpus > 1 the units of the tiled CausalVAE decode are dealt over the ranks and gathered once (the reference decodes
        # every tile on every rank: pipeline_open_sora_plan.py:1184-1190 under engine.py:85-95); False = the reference's behaviour
        self.shard_vae_decode = bool(extra.pop("shard_vae_decode", True))
        if extra:
            raise TypeError(f"unexpected OpenSoraPlanConfig kwargs: {sorted(extra)}")


class EulerAncestralDiscreteScheduler:
    """diffusers EulerAncestralDiscreteScheduler with its defaults, as pipeline_open_sora_plan.py:306,1082,1110,1161 uses it.
    UNPINNED restatement: diffusers is third-party, not vendored by the reference and not installed here, so no fixture of the class
    backs this one; it is held to the closed form below (tests/test_osp_pipeline_cpu.py).

      __init__        1000 training steps, linear betas 1e-4 .. 0.02 (fp32), sigma = sqrt((1 - abar) / abar), timestep_spacing
                      "linspace", epsilon prediction
      set_timesteps   t = linspace(0, 999, n)[::-1] (fp32), sigmas = interp(t, arange(1000), sigma) with 0 appended (fp32)
      init_noise_sigma  max(sigmas)
      scale_model_input  sample / sqrt(sigma^2 + 1) at the step of ``timestep``
      step            sigma_up = sqrt(s_to^2 (s_from^2 - s_to^2) / s_from^2), sigma_down = sqrt(s_to^2 - sigma_up^2),
                      prev = sample + (sigma_down - s_from) eps + sigma_up noise in fp32; the step index advances by one."""

    order = 1

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.0001, beta_end: float = 0.02,
                 beta_schedule: str = "linear", prediction_type: str = "epsilon", timestep_spacing: str = "linspace",
                 steps_offset: int = 0, rescale_betas_zero_snr: bool = False):
        if beta_schedule != "linear" or prediction_type != "epsilon" or timestep_spacing != "linspace" or rescale_betas_zero_snr:
            raise NotImplementedError("EulerAncestralDiscreteScheduler: the defaults the Open-Sora-Plan pipeline constructs it with "
                                      "(linear betas, epsilon prediction, linspace spacing) are what is built")
        self.num_train_timesteps = num_train_timesteps
        self.betas = torch.linspace(beta_start, beta_end, num_train_timesteps, dtype=torch.float32)
        self.alphas_cumprod = torch.cumprod(1.0 - self.betas, dim=0)
        self._train_sigmas = (((1 - self.alphas_cumprod) / self.alphas_cumprod) ** 0.5).numpy()
        self.sigmas = torch.from_numpy(np.concatenate([self._train_sigmas[::-1], [0.0]]).astype(np.float32))
        self.timesteps = torch.from_numpy(np.linspace(0, num_train_timesteps - 1, num_train_timesteps, dtype=float)[::-1].copy())
        self.num_inference_steps = None
        self._step_index = None

    step_index = property(lambda self: self._step_index)
    init_noise_sigma = property(lambda self: float(self.sigmas.max()))

    def set_timesteps(self, num_inference_steps: int, device=None):
        self.num_inference_steps = num_inference_steps
        N = self.num_train_timesteps
        t = np.linspace(0, N - 1, num_inference_steps, dtype=np.float32)[::-1].copy()
        s = np.interp(t, np.arange(0, N), self._train_sigmas)
        self.sigmas = torch.from_numpy(np.concatenate([s, [0.0]]).astype(np.float32))
        self.timesteps = torch.from_numpy(t)
        self._step_index = None

    def _index_for(self, timestep) -> int:
        hits = (self.timesteps == float(timestep)).nonzero()
        return int(hits[1 if len(hits) > 1 else 0])

    def in_scale(self, i: int) -> float:
        """1 / sqrt(sigma_i^2 + 1): what scale_model_input multiplies the sample of step ``i`` by (1 past the last step)."""
        return 1.0 / math.sqrt(float(self.sigmas[i]) ** 2 + 1.0)

    def step_coeffs(self, i: int) -> Tuple[float, float]:
        """(dt, sigma_up) of step ``i`` in Python doubles from the fp32 sigmas."""
        s_from, s_to = float(self.sigmas[i]), float(self.sigmas[i + 1])
        sigma_up = math.sqrt(s_to ** 2 * (s_from ** 2 - s_to ** 2) / s_from ** 2)
        sigma_down = math.sqrt(s_to ** 2 - sigma_up ** 2)
        return sigma_down - s_from, sigma_up

    def scale_model_input(self, sample, timestep):
        if self._step_index is None:
            self._step_index = self._index_for(timestep)
        return sample / ((self.sigmas[self._step_index] ** 2 + 1) ** 0.5)

    def step(self, model_output, timestep, sample, generator=None, return_dict: bool = True):
        if self._step_index is None:
            self._step_index = self._index_for(timestep)
        dt, sigma_up = self.step_coeffs(self._step_index)
        wide = torch.promote_types(sample.dtype, torch.float32)        # diffusers upcasts to fp32; a float64 sample stays float64
        noise = torch.randn(model_output.shape, generator=generator, dtype=model_output.dtype,
                            device=generator.device if generator is not None else "cpu").to(model_output.device)
        prev = (sample.to(wide) + model_output.to(wide) * dt + noise.to(wide) * sigma_up).to(model_output.dtype)
        self._step_index += 1
        return (prev,)


class OpenSoraPlanPipeline(VideoSysPipeline):
    model_cpu_offload_seq = "text_encoder->transformer->vae"
    _optional_components = ["tokenizer", "text_encoder", "vae", "transformer", "scheduler"]

    def __init__(self, config: OpenSoraPlanConfig, tokenizer=None, text_encoder=None, vae=None, transformer=None, scheduler=None,
                 device: torch.device = torch.device("cuda"), dtype: torch.dtype = torch.bfloat16):
        """pipeline_open_sora_plan.py:257-341, same parameter order.  Components left at None are read from ``config.transformer`` when
        that is a LOCAL checkpoint directory (``<transformer_type>/``, ``vae/``); ``"synthetic:<seed>"`` builds seeded weights."""
        import torch.distributed as dist

        world = dist.get_world_size() if dist.is_initialized() else 1
        if config.num_gpus != world:      # before any component is read
            raise _NoGroupOfThatSize(f"OpenSoraPlanPipeline: num_gpus={config.num_gpus}, but the process group initialised in this process "
                                     f"has {world} rank(s): a pipeline is one rank of a group of num_gpus processes (VideoSysEngine "
                                     f"starts them; or dsp.initialize in every process)")
        self._config = config
        self._dtype = self._check_dtype(dtype)
        self._device = self._resolve_device(device, "OpenSoraPlanPipeline")
        name = config.transformer
        synthetic = isinstance(name, str) and name.startswith("synthetic:")
        seed = int(name.split(":", 1)[1]) if synthetic else 1202
        if transformer is None or is_foreign_module(transformer, OpenSoraT2V):
            file_cfg, sd = module_state(transformer) if transformer is not None else read_component(name, config.transformer_type)
            tcfg = dict(_V120_GEOMETRY[config.transformer_type])
            tcfg.update(ctor_kwargs(OpenSoraT2V.__init__, file_cfg))
            tcfg.update(config.transformer_config or {})
            transformer = OpenSoraT2V(**tcfg, device=self._device)
            if sd is None:
                c = transformer.config
                sd = synth_state_dict(num_layers=c.num_layers, num_heads=c.num_attention_heads, caption_channels=c.caption_channels,
                                      in_channels=c.in_channels, out_channels=c.out_channels, patch_size=c.patch_size, seed=seed)
            transformer.load_state_dict(sd)
        self.transformer = transformer
        if transformer.config.out_channels != 2 * transformer.config.in_channels:
            raise NotImplementedError("OpenSoraPlanPipeline: the step kernel drops a learned-sigma half (out_channels = 2 in_channels)")
        self.transformer.force_images = False
        if scheduler is None:
            scheduler = EulerAncestralDiscreteScheduler()
        self.scheduler = self._check_scheduler(scheduler, "step_coeffs", "videosys_amd.pipeline_open_sora_plan.EulerAncestralDiscreteScheduler")
        if vae is None:
            vae = self._load_vae(name, seed if synthetic else None)
        elif is_foreign_module(vae):
            vae = self._vae_from_state(module_state(vae)[1])
        self.vae = vae
        if self.vae is not None:
            if config.enable_tiling:                  # (:309-315)
                self.vae.vae.enable_tiling()
                self.vae.vae.tile_overlap_factor = config.tile_overlap_factor
                self.vae.vae.tile_sample_min_size = 512
                self.vae.vae.tile_latent_min_size = 64
                self.vae.vae.tile_sample_min_size_t = 29
                self.vae.vae.tile_latent_min_size_t = 8
            self.vae.vae_scale_factor = [4, 8, 8]
        self.vae_scale_factor = [4, 8, 8]
        if text_encoder is None and isinstance(config.text_encoder, str) and \
                (os.path.isdir(config.text_encoder) or config.text_encoder.startswith("synthetic:")):
            text_encoder = config.text_encoder
        self.text_encoder = self._build_text_encoder(text_encoder, tokenizer)
        pab.set_pab_manager(config.pab_config if config.enable_pab else None)
        self._steps = program.StepCache()   # (geometry, text shape, PAB pattern) -> (Program, pred)
        self._step_bufs = None
        self.pab_trace: List[list] = []     # PAB on: per step of the last generate(), every block's (spatial, cross) decision
        self._set_parallel()
        self._init_stages(config.cpu_offload, self._device, text_encoder=getattr(self.text_encoder, "encoder", None),
                          transformer=self.transformer, vae=getattr(self.vae, "vae", None))

    tokenizer = property(lambda self: getattr(self.text_encoder, "tokenizer", None))
    step_stats = program.stats_property("_steps")

    TEXT_VOCAB, TEXT_MAX_LENGTH = MT5_VOCAB, 512          # (the v1.1 pipeline: T5 v1.1's vocabulary, 300 tokens)

    def _build_text_encoder(self, spec, tokenizer):
        """mT5 = t5.T5Encoder(vocab_size=250112); ``"synthetic:<seed>"``: XXL geometry when the transformer takes 4096-wide captions,
        else 2 layers (tests) of the caption width rounded up to the encoder's 128-column granularity, of which the first
        ``caption_channels`` columns are the caption; the byte tokenizer over the mT5 vocabulary."""
        from .t5 import ByteTokenizer, T5Encoder, T5TextEncoder

        d = self.transformer.config.caption_channels
        if isinstance(spec, str) and spec.startswith("synthetic:"):
            dm = -(-d // 128) * 128
            geo = dict(d_model=4096, d_ff=10240, num_layers=24, num_heads=64) if d == 4096 else \
                dict(d_model=dm, d_ff=2 * dm, num_layers=2, num_heads=max(dm // 64, 2))
            enc = T5Encoder(device=self._device, vocab_size=self.TEXT_VOCAB, **geo).init_random_(int(spec.split(":", 1)[1]))

            class Narrow(T5TextEncoder):
                def __call__(self, prompts):
                    emb, mask = super().__call__(prompts)
                    return emb[..., :d].contiguous(), mask

            return Narrow(enc, tokenizer or ByteTokenizer(self.TEXT_VOCAB), max_length=self.TEXT_MAX_LENGTH)
        return build_text_encoder(spec, tokenizer, device=self._device, caption_channels=d, max_length=self.TEXT_MAX_LENGTH)

    def _vae_from_state(self, sd):
        from .vae_open_sora_plan import CausalVAEModelWrapper

        return CausalVAEModelWrapper(sd, device=self._device, **(self._config.vae_config or {}))

    def _load_vae(self, name, synthetic_seed):
        """:289-290 CausalVAEModelWrapper(config.transformer, subfolder="vae"): a local ``vae/`` directory, or seeded weights for
        ``"synthetic:<seed>"``; None when neither is there (generate() then returns latents)."""
        from .vae_open_sora_plan import CausalVAEModelWrapper

        if synthetic_seed is not None:
            return CausalVAEModelWrapper(f"synthetic:{synthetic_seed}", device=self._device, **(self._config.vae_config or {}))
        if not isinstance(name, str):
            return None
        sd = read_component(name, "vae")[1]
        return self._vae_from_state(sd) if sd is not None else None

    def _set_parallel(self, dp_size: Optional[int] = None, sp_size: Optional[int] = None, enable_cp: Optional[bool] = False,
                      parallel_mgr=None):
        """pipeline_open_sora_plan.py:349-363: sp = world size unless given.  The transformer shards the video tokens (open_sora_plan.py:
        every rank calls generate() with the same seed, draws the same latents and per-step noise, and gets the full prediction, the
        model gathering it inside); the text encoder stays replicated, the tiled CausalVAE decode is shared over the same group
        (``_decode_group``).  ``parallel_mgr`` (an extension): an injected manager instead of the process group, as the transformer
        takes it."""
        self._steps.clear()                # a recorded step belongs to the sharding it was recorded under
        if parallel_mgr is not None:
            return self.transformer.enable_parallel(parallel_mgr=parallel_mgr)
        self.transformer.enable_parallel(*self._parallel_sizes(sp_size), enable_cp)    # (at one rank too)

    # ------------------------------------------------------------------------------------------------ text side
    def mask_text_embeddings(self, emb, mask):
        """pipeline_open_sora_plan.py:366-372."""
        if emb.shape[0] == 1:
            keep_index = int(mask.sum().item())
            return emb[:, :, :keep_index, :], keep_index
        return emb * mask[:, None, :, None].to(device=emb.device, dtype=emb.dtype), emb.shape[2]

    def _text_preprocessing(self, text, clean_caption: bool = False):
        """:755-767: a string or a list of strings -> a list; the IF caption cleaner twice, or lower + strip."""
        from .caption import text_preprocessing

        text = [text] if not isinstance(text, (list, tuple)) else text
        return [text_preprocessing(t, clean_caption, mid_strip=False) for t in text]

    def _clean_caption(self, caption):
        """:770-886 (one application)."""
        from .caption import clean_caption

        return clean_caption(caption, mid_strip=False)

    def encode_prompt(self, *args, **kwargs):
        """:375-536 is the v1.1 path (T5 v1.1 at 300 tokens, embeddings cut to the prompt): OpenSoraPlanV110Pipeline.encode_prompt."""
        raise NotImplementedError("OpenSoraPlanPipeline.encode_prompt is the v1.1 text path (OpenSoraPlanV110Pipeline.encode_prompt); "
                                  "v1.2 uses encode_prompt_v120")

    def _encode(self, prompts, max_length):
        if self.text_encoder is None:
            raise RuntimeError("no text encoder attached: pass prompt_embeds / negative_prompt_embeds with their attention masks")
        self._enter_stage("text_encoder")
        if hasattr(self.text_encoder, "max_length"):
            self.text_encoder.max_length = max_length
        emb, mask = self.text_encoder(list(prompts))
        return emb.reshape(emb.shape[0], emb.shape[-2], emb.shape[-1]), mask.reshape(emb.shape[0], -1)

    def encode_prompt_v120(self, prompt, do_classifier_free_guidance: bool = True, negative_prompt: str = "",
                           num_images_per_prompt: int = 1, device=None, prompt_embeds: Optional[torch.Tensor] = None,
                           negative_prompt_embeds: Optional[torch.Tensor] = None, prompt_attention_mask: Optional[torch.Tensor] = None,
                           negative_prompt_attention_mask: Optional[torch.Tensor] = None, clean_caption: bool = False,
                           max_sequence_length: int = 120, **kwargs):
        """:538-673 -> (prompt_embeds [B, L, d], prompt_attention_mask [B, L], negative_prompt_embeds, negative mask): every prompt
        padded to ``max_sequence_length`` with its mask, the negative prompt encoded once per prompt at the same length."""
        device = device or self._device
        if prompt is not None and isinstance(prompt, str):
            batch_size = 1
        elif prompt is not None and isinstance(prompt, list):
            batch_size = len(prompt)
        else:
            batch_size = prompt_embeds.shape[0]
        if prompt_embeds is None:
            prompt_embeds, prompt_attention_mask = self._encode(self._text_preprocessing(prompt, clean_caption), max_sequence_length)
        prompt_embeds = prompt_embeds.to(dtype=self._dtype, device=device)
        bs_embed, seq_len, _ = prompt_embeds.shape
        prompt_embeds = prompt_embeds.repeat(1, num_images_per_prompt, 1).view(bs_embed * num_images_per_prompt, seq_len, -1)
        prompt_attention_mask = prompt_attention_mask.to(device).view(bs_embed, -1).repeat(num_images_per_prompt, 1)
        if do_classifier_free_guidance and negative_prompt_embeds is None:
            uncond = self._text_preprocessing([negative_prompt] * batch_size, clean_caption)
            negative_prompt_embeds, negative_prompt_attention_mask = self._encode(uncond, prompt_embeds.shape[1])
        if do_classifier_free_guidance:
            seq_len = negative_prompt_embeds.shape[1]
            negative_prompt_embeds = negative_prompt_embeds.to(dtype=self._dtype, device=device)
            negative_prompt_embeds = negative_prompt_embeds.repeat(1, num_images_per_prompt, 1).view(batch_size * num_images_per_prompt, seq_len, -1)
            negative_prompt_attention_mask = negative_prompt_attention_mask.to(device).view(bs_embed, -1).repeat(num_images_per_prompt, 1)
        else:
            negative_prompt_embeds = negative_prompt_attention_mask = None
        return prompt_embeds, prompt_attention_mask, negative_prompt_embeds, negative_prompt_attention_mask

    def prepare_extra_step_kwargs(self, generator, eta):
        """:676-691: the keywords the scheduler's ``step`` takes beyond (model_output, t, sample)."""
        names = set(inspect.signature(self.scheduler.step).parameters.keys())
        kw = {}
        if "eta" in names:
            kw["eta"] = eta
        if "generator" in names:
            kw["generator"] = generator
        return kw

    def check_inputs(self, prompt, height, width, negative_prompt, callback_steps, prompt_embeds=None, negative_prompt_embeds=None,
                     prompt_attention_mask=None, negative_prompt_attention_mask=None):
        """:693-752: the argument combinations the reference refuses, with its ValueErrors."""
        if height % 8 != 0 or width % 8 != 0:
            raise ValueError(f"`height` and `width` have to be divisible by 8 but are {height} and {width}.")
        if callback_steps is None or not isinstance(callback_steps, int) or callback_steps <= 0:
            raise ValueError(f"`callback_steps` has to be a positive integer but is {callback_steps} of type {type(callback_steps)}.")
        both = "Please make sure to only forward one of the two."
        if prompt is not None and prompt_embeds is not None:
            raise ValueError(f"Cannot forward both `prompt`: {prompt} and `prompt_embeds`. {both}")
        elif prompt is None and prompt_embeds is None:
            raise ValueError("Provide either `prompt` or `prompt_embeds`. Cannot leave both `prompt` and `prompt_embeds` undefined.")
        elif prompt is not None and (not isinstance(prompt, str) and not isinstance(prompt, list)):
            raise ValueError(f"`prompt` has to be of type `str` or `list` but is {type(prompt)}")
        if prompt is not None and negative_prompt_embeds is not None:
            raise ValueError(f"Cannot forward both `prompt`: {prompt} and `negative_prompt_embeds`. {both}")
        if negative_prompt is not None and negative_prompt_embeds is not None:
            raise ValueError(f"Cannot forward both `negative_prompt`: {negative_prompt} and `negative_prompt_embeds`. {both}")
        if prompt_embeds is not None and negative_prompt_embeds is not None:
            if prompt_embeds.shape != negative_prompt_embeds.shape:
                raise ValueError("`prompt_embeds` and `negative_prompt_embeds` must have the same shape when passed directly, but"
                                 f" got: `prompt_embeds` {prompt_embeds.shape} != `negative_prompt_embeds` {negative_prompt_embeds.shape}.")
            if prompt_attention_mask.shape != negative_prompt_attention_mask.shape:
                raise ValueError("`prompt_attention_mask` and `negative_prompt_attention_mask` must have the same shape when passed "
                                 f"directly, but got: `prompt_attention_mask` {prompt_attention_mask.shape} != "
                                 f"`negative_prompt_attention_mask` {negative_prompt_attention_mask.shape}.")

    def latent_shape(self, batch_size, num_channels_latents, num_frames, height, width):
        sf = self.vae_scale_factor
        nf = int(num_frames)
        t = (math.ceil((nf - 1) / sf[0]) + 1) if nf % 2 == 1 else math.ceil(nf / sf[0])
        return (batch_size, num_channels_latents, t, math.ceil(int(height) / sf[1]), math.ceil(int(width) / sf[2]))

    def prepare_latents(self, batch_size, num_channels_latents, num_frames, height, width, dtype, device, generator, latents=None):
        """:888-908: start latents [B, C, T_lat, h / 8, w / 8] * init_noise_sigma, drawn from ``generator`` unless handed in."""
        if latents is None:
            latents = _randn(self.latent_shape(batch_size, num_channels_latents, num_frames, height, width), generator, dtype)
        return latents.to(device=device, dtype=dtype) * self.scheduler.init_noise_sigma

    # ------------------------------------------------------------------------------------------------ denoise step
    def _pab_pattern(self, t_int):
        """The (spatial, cross) decisions the model's blocks will make at this step and the counters they leave, WITHOUT touching the
        blocks' state (pab decisions are functions of the timestep and the counter)."""
        mgr = pab.PAB_MANAGER
        return [(mgr.if_broadcast_spatial(t_int, st.attn_count), mgr.if_broadcast_cross(t_int, st.cross_count))
                for st in self.transformer.states]

    def _model(self, xin, t, enc, mask):
        nb = xin.shape[0]
        return self.transformer(xin, timestep=torch.full((nb,), float(t)), encoder_hidden_states=enc, encoder_attention_mask=mask,
                                added_cond_kwargs={"resolution": None, "aspect_ratio": None}, return_dict=False)[0]

    def _issue_model(self, xin, t, enc, mask):
        """One CFG model call -> fp32 [2B, 2C, T, h, w]: eagerly (``transformer.use_programs`` False), or through the launch program
        recorded for this (geometry, text shape, PAB decision pattern)."""
        tr = self.transformer
        use_pab = pab.enable_pab()
        plan = self._pab_pattern(int(t)) if use_pab else None
        if use_pab:
            self.pab_trace.append([(s[0], c[0]) for s, c in plan])
        if not getattr(tr, "use_programs", True):
            return self._steps.eager(lambda: self._model(xin, t, enc, mask))
        key = (tuple(xin.shape), tuple(enc.shape), None if plan is None else tuple((s[0], c[0]) for s, c in plan))

        def refresh(pred):
            tr.step_timesteps(xin.shape[0]).fill_(float(t))       # the one per-step input besides the latents
            if plan is not None:                                   # the counters the eager call would have left
                for st, (s, c) in zip(tr.states, plan):
                    st.attn_count, st.cross_count = s[1], c[1]

        return self._steps.run(key, lambda: self._model(xin, t, enc, mask), refresh)

    def _buffers(self, z0, enc, mask):
        """Resident inputs of a step — latents z fp32 [B, C, T, h, w], the model input as the step kernel leaves it (bf16 [2B, ...])
        and as the patch embedding reads it (fp32), the text — kept across generate() calls of one geometry so that the recorded
        programs (which hold their addresses) stay valid; a new prompt of the same shape refills them."""
        b = self._step_bufs
        if b is not None and b["z"].shape == z0.shape and b["enc"].shape == enc.shape and b["mask"].shape == mask.shape:
            b["z"].copy_(z0)
            b["enc"].copy_(enc)
            b["mask"].copy_(mask)
            return b
        self._steps.clear()
        z = z0.to(device=self._device, dtype=torch.float32).contiguous().clone()
        two = (2 * z.shape[0],) + tuple(z.shape[1:])
        self._step_bufs = dict(z=z, model_in=torch.empty(two, dtype=torch.bfloat16, device=self._device),
                               xin=torch.empty(two, dtype=torch.float32, device=self._device),
                               enc=enc.contiguous().clone(), mask=mask.contiguous().clone())
        return self._step_bufs

    def _noise(self, shape, generator):
        if generator is not None and generator.device.type != "cuda":
            return torch.randn(shape, generator=generator, dtype=torch.float32).to(self._device)
        return torch.randn(shape, generator=generator, dtype=torch.float32, device=self._device)

    @torch.no_grad()
    def generate(self, prompt: Union[str, List[str]] = None, negative_prompt: str = "", num_inference_steps: int = 100,
                 guidance_scale: float = 7.5, num_images_per_prompt: Optional[int] = 1, eta: float = 0.0, seed: int = -1,
                 generator: Optional[Union[torch.Generator, List[torch.Generator]]] = None, latents: Optional[torch.FloatTensor] = None,
                 prompt_embeds: Optional[torch.FloatTensor] = None, prompt_attention_mask: Optional[torch.FloatTensor] = None,
                 negative_prompt_embeds: Optional[torch.FloatTensor] = None,
                 negative_prompt_attention_mask: Optional[torch.FloatTensor] = None, output_type: Optional[str] = "pil",
                 return_dict: bool = True, callback: Optional[Callable[[int, int, torch.FloatTensor], None]] = None,
                 callback_steps: int = 1, clean_caption: bool = True, mask_feature: bool = True,
                 enable_temporal_attentions: bool = True, verbose: bool = True,
                 max_sequence_length: int = 512) -> Union[VideoSysPipelineOutput, Tuple]:
        """pipeline_open_sora_plan.py:911-1182 with the reference's parameters and defaults (module docstring for the sampler).
        ``output_type="latents"`` returns the fp32 latents (also what comes back when no VAE is attached); anything else the uint8
        video [B, num_frames, height, width, 3] on the CPU.  ``eta`` is ignored as the reference's scheduler ignores it;
        ``mask_feature`` and ``enable_temporal_attentions`` have nothing to act on in v1.2 (:1053-1071, the 3-D attention)."""
        if isinstance(generator, (list, tuple)):
            raise NotImplementedError("a list of generators: the per-step noise is drawn from one generator")
        tc = self.transformer.config
        height, width = tc.sample_size[0] * self.vae_scale_factor[1], tc.sample_size[1] * self.vae_scale_factor[2]
        num_frames = self._config.num_frames
        pab.update_steps(num_inference_steps)
        self.check_inputs(prompt, height, width, negative_prompt if prompt is not None else None, callback_steps, prompt_embeds,
                          negative_prompt_embeds, prompt_attention_mask, negative_prompt_attention_mask)
        seed = self._set_seed(seed)
        if prompt is not None and isinstance(prompt, str):
            batch_size = 1
        elif prompt is not None and isinstance(prompt, list):
            batch_size = len(prompt)
        else:
            batch_size = prompt_embeds.shape[0]
        do_cfg = guidance_scale > 1.0
        prompt_embeds, prompt_attention_mask, negative_prompt_embeds, negative_prompt_attention_mask = self.encode_prompt_v120(
            prompt, do_cfg, negative_prompt=negative_prompt, num_images_per_prompt=num_images_per_prompt, device=self._device,
            prompt_embeds=prompt_embeds, negative_prompt_embeds=negative_prompt_embeds, prompt_attention_mask=prompt_attention_mask,
            negative_prompt_attention_mask=negative_prompt_attention_mask, clean_caption=clean_caption,
            max_sequence_length=max_sequence_length)
        if do_cfg:                                                                                     # (:1072-1075)
            enc = torch.cat([negative_prompt_embeds, prompt_embeds], dim=0)
            mask = torch.cat([negative_prompt_attention_mask, prompt_attention_mask], dim=0)
        else:                                                                                          # (module docstring)
            enc, mask = torch.cat([prompt_embeds, prompt_embeds], dim=0), torch.cat([prompt_attention_mask, prompt_attention_mask], dim=0)
        enc, mask = enc[:, None], mask[:, None]                                                        # b l d -> b 1 l d (:1127-1131)
        timesteps, num_inference_steps = retrieve_timesteps(self.scheduler, num_inference_steps, self._device, None)
        self._enter_stage("transformer")
        self.transformer.reset_pab_state()
        self.pab_trace = []
        if generator is None:
            generator = torch.Generator(device=self._device).manual_seed(seed)
        z0 = self.prepare_latents(batch_size * num_images_per_prompt, tc.in_channels, num_frames, height, width, torch.float32,
                                  self._device, generator, latents)
        b = self._buffers(z0, enc, mask)
        z, model_in, xin, enc, mask = b["z"], b["model_in"], b["xin"], b["enc"], b["mask"]
        # the text K / V are step-invariant: made resident here (a no-op for an unchanged prompt), so that no recorded step holds them
        # and a replayed one finds this prompt's
        self.transformer._encode_text(enc, mask)
        sch = self.scheduler
        # scale_model_input of the first step (:1109-1110) on the CFG pair; the later ones come out of the step kernel
        model_in.copy_((z * sch.in_scale(0)).to(torch.bfloat16).repeat(2, 1, 1, 1, 1))
        g = guidance_scale if do_cfg else 1.0
        for i, t in progress_wrap(list(enumerate(timesteps.tolist())), verbose):
            xin.copy_(model_in)
            pred = self._issue_model(xin, t, enc, mask)
            dt, sigma_up = sch.step_coeffs(i)
            noise = self._noise(z.shape, generator) if sigma_up > 0.0 else None
            oops.cfg_ancestral_step(z, pred, noise, model_in, g, dt, sigma_up, sch.in_scale(i + 1))
            if callback is not None and i % callback_steps == 0:                                       # (:1164-1167)
                callback(i, t, z)
        dsp.check_exchange(self.transformer)     # a timed-out peer-to-peer exchange raises here, before anything is decoded
        if self.vae is None or output_type in ("latent", "latents"):
            return self._leave(z.clone(), return_dict)
        self._enter_stage("vae")
        return self._leave(self.decode_latents(z)[:, :num_frames, :height, :width], return_dict)

    def decode_latents(self, latents):
        """:1184-1190: the VAE on the bf16 latents, then ``((video / 2 + 0.5).clamp(0, 1) * 255).to(uint8)`` on the bf16 tensor
        (vsys_pixels_to_u8_trunc) -> uint8 [B, T, H, W, 3] on the CPU.  Under sequence parallelism the tiles of the decode are shared
        by the ranks (``_decode_group``); the uint8 pass runs after the blend, on every rank."""
        from .ops import VaeGrid

        grp = self._decode_group()
        kw = {} if grp is None else {"group": grp}                           # (an injected VAE is called as the reference calls it)
        video = self.vae.decode(latents.to(torch.bfloat16), **kw)            # [B, T, 3, H, W] bf16
        B, T, _, H, W = video.shape
        out = torch.empty(B * T, H, W, 3, dtype=torch.uint8, device=video.device)
        rows = torch.zeros(T * H * W, 4, dtype=torch.bfloat16, device=video.device)
        for bi in range(B):
            rows[:, :3] = video[bi].permute(0, 2, 3, 1).reshape(-1, 3)
            oops.pixels_to_u8_trunc(rows, VaeGrid(T, 1, H, W, 0, 0), out, bi * T)
        return out.view(B, T, H, W, 3).cpu()

    def save_video(self, video, output_path):
        from .utils import save_video

        return save_video(video, output_path, fps=24)        # (:1192-1193)


# OpenSoraT2V constructor keywords of the published v1.2 checkpoints (OpenSoraT2V_ROPE_L_122, open_sora_plan_v120_transformer_3d.py,
# with the sample sizes of the four transformer types: latent frames x (height / 8) x (width / 8))
def _geometry(frames_lat, h, w):
    return dict(num_layers=32, attention_head_dim=96, num_attention_heads=24, patch_size_t=1, patch_size=2, norm_type="ada_norm_single",
                caption_channels=4096, cross_attention_dim=2304, in_channels=4, out_channels=8, attention_bias=True,
                sample_size=(h, w), sample_size_t=frames_lat, activation_fn="gelu-approximate", norm_elementwise_affine=False,
                norm_eps=1e-6, use_rope=True)


_V120_GEOMETRY = {"29x480p": _geometry(8, 60, 80), "93x480p": _geometry(24, 60, 80), "29x720p": _geometry(8, 90, 160),
                  "93x720p": _geometry(24, 90, 160)}


# ---------------------------------------------------------------------------------------------------- the v1.1 names
_V110_NAMES = ("OpenSoraPlanV110PABConfig", "OpenSoraPlanV110Config", "OpenSoraPlanV110Pipeline", "PNDMScheduler")


def __getattr__(name):
    """The v1.1 classes live in pipeline_open_sora_plan_v110.py, which imports this module: resolved on first use."""
    if name in _V110_NAMES:
        from . import pipeline_open_sora_plan_v110 as v110

        return getattr(v110, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
