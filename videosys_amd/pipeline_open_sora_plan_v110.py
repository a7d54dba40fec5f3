"""Open-Sora-Plan v1.1 pipeline plug-in — the ``version == "v110"`` route of videosys/pipelines/open_sora_plan/pipeline_open_sora_plan.py
(OpenSoraPlanV110PABConfig :41-100, OpenSoraPlanConfig :123-225, OpenSoraPlanPipeline :228-1193): prompt -> T5 v1.1 embeddings at 300
tokens, cut to the prompt or multiplied by the mask (``encode_prompt`` :375-536) -> PNDM sampling with LatteT2V (open_sora_plan_v110.py)
-> v1.1 CausalVAE decode (vae_open_sora_plan_v110.py) -> uint8 video [B, T, H, W, 3].

Classes of its own.  The reference switches on ``OpenSoraPlanConfig(version=)``; here ``OpenSoraPlanConfig(version="v110")`` and
``OpenSoraPlanPipeline.encode_prompt`` keep raising (pinned by tests/test_osp_pipeline_cpu.py), and the v1.1 route is
``OpenSoraPlanV110Config`` + ``OpenSoraPlanV110Pipeline`` (DESIGN.md "known wart": a later change that may edit that test folds the
two).  ``OpenSoraPlanV110Config`` takes the reference's keywords minus ``version`` and drops into ``VideoSysEngine``.

Sampler.  ``PNDMScheduler`` below restates diffusers' class with its defaults (UNPINNED: its docstring).  A generate() of n steps makes
n + 9 model calls (twelve Runge-Kutta warm-up calls, n - 3 linear multistep calls) on the CFG batch [negative | prompt]; after each
call ONE launch of ``vsys_cfg_pndm_step`` does the guidance combine, the drop of the learned-sigma half, the scheduler update and the
next call's bf16 model input.  Host side of that launch (``generate``, ``_buffers``): the latents ping-pong between two fp32 buffers during the
warm-up (the buffer that is not written is the scheduler's ``cur_sample``) and are updated in place afterwards; the history of combined
predictions is a ring of four buffers; the Runge-Kutta accumulator is a buffer of its own.  The launch is issued eagerly after the model
call, so the rotating pointers never enter a recorded program.  The model call itself is recorded once per (geometry, text length) and
replayed with the timestep written into the transformer's resident buffer; the step-invariant text K / V of the cross-attentions are
made once per prompt, outside the recording (``_prepare_text``), as the v1.2 pipeline does.  With PAB on, every call is issued eagerly
from the host — about 450 launches per call — because the decisions of the v1.1 PAB configuration (spatial, temporal, cross and both
MLP tables; ``_pab_pattern`` computes them for ``pab_trace``) are not folded into a program key yet; no time under PAB has been
measured, so PAB on may be slower than PAB off here.
Without guidance (``guidance_scale <= 1``) the model runs on [prompt | prompt] at guidance 1: u + 1 (c - u) with u = c is c exactly."""
from __future__ import annotations

import os
from typing import Callable, List, Optional, Tuple, Union

import numpy as np
import torch

from . import open_sora_plan_v110_ops as vops
from . import dsp, pab, program
from .open_sora_plan_v110 import LatteT2V, synth_state_dict
from .pab import PABConfig
from .pipeline import VideoSysPipelineOutput, is_foreign_module, module_state
from .pipeline_open_sora_plan import OpenSoraPlanPipeline
from .utils import ctor_kwargs, progress_wrap, read_component

V110_TYPES = ("65x512x512", "221x512x512")
MAX_LENGTH = 300                     # encode_prompt :427


def _mlp_table():
    return {t: {"block": [0, 1, 2, 3, 4, 5, 6], "skip_count": 2} for t in range(738, 425, -24)}


class OpenSoraPlanV110PABConfig(PABConfig):
    """pipeline_open_sora_plan.py:41-100 — identical defaults (both MLP tables: timesteps 738, 714, ..., 426, blocks 0..6, skip 2)."""

    def __init__(self, spatial_broadcast: bool = True, spatial_threshold: list = [100, 850], spatial_range: int = 2,
                 temporal_broadcast: bool = True, temporal_threshold: list = [100, 850], temporal_range: int = 4,
                 cross_broadcast: bool = True, cross_threshold: list = [100, 850], cross_range: int = 6, mlp_broadcast: bool = True,
                 mlp_spatial_broadcast_config: dict = _mlp_table(), mlp_temporal_broadcast_config: dict = _mlp_table()):
        super().__init__(spatial_broadcast=spatial_broadcast, spatial_threshold=spatial_threshold, spatial_range=spatial_range,
                         temporal_broadcast=temporal_broadcast, temporal_threshold=temporal_threshold, temporal_range=temporal_range,
                         cross_broadcast=cross_broadcast, cross_threshold=cross_threshold, cross_range=cross_range,
                         mlp_broadcast=mlp_broadcast, mlp_spatial_broadcast_config=mlp_spatial_broadcast_config,
                         mlp_temporal_broadcast_config=mlp_temporal_broadcast_config)


class OpenSoraPlanV110Config:
    """pipeline_open_sora_plan.py:123-225 at ``version="v110"`` — the reference's keywords and defaults minus ``version``.
    ``transformer``: a LOCAL checkpoint directory in the published layout (``<transformer_type>/``, ``vae/``), ``"synthetic:<seed>"``
    (seeded transformer and CausalVAE weights), or a hub id (cannot be fetched here: the published geometry with seeded transformer
    weights, no VAE).  Extensions, for tests: ``transformer_config`` / ``vae_config`` (geometry overrides) and ``num_frames``."""

    version = "v110"

    def __init__(self, transformer_type: str = "65x512x512", transformer: str = None, text_encoder: str = None, num_gpus: int = 1,
                 cpu_offload: bool = False, enable_tiling: bool = True, tile_overlap_factor: float = 0.25, enable_pab: bool = False,
                 pab_config: PABConfig = None, **extra):
        self.pipeline_cls = OpenSoraPlanV110Pipeline
        assert transformer_type in V110_TYPES, f"transformer_type must be one of {V110_TYPES}"
        self.transformer_type = transformer_type
        self.num_frames = int(extra.pop("num_frames", None) or transformer_type.split("x")[0])
        self.text_encoder = text_encoder or "DeepFloyd/t5-v1_1-xxl"
        self.transformer = transformer or "LanguageBind/Open-Sora-Plan-v1.1.0"
        self.num_gpus = num_gpus
        self.cpu_offload = cpu_offload
        self.enable_tiling = enable_tiling
        self.tile_overlap_factor = tile_overlap_factor
        self.enable_pab = enable_pab
        self.pab_config = OpenSoraPlanV110PABConfig() if (enable_pab and pab_config is None) else pab_config
        self.transformer_config = extra.pop("transformer_config", None)
        self.vae_config = extra.pop("vae_config", None)
        if extra:
            raise TypeError(f"unexpected OpenSoraPlanV110Config kwargs: {sorted(extra)}")


class PNDMScheduler:
    """diffusers PNDMScheduler with its defaults, as pipeline_open_sora_plan.py:302-304,1079-1080,1161 uses it.  UNPINNED restatement:
    diffusers is third-party, not vendored by the reference and not installed here, so no fixture of the class backs this one; it is
    held to the algorithm below and to the closed form of an exact epsilon (tests/test_osp_v110_pipeline_cpu.py).

      __init__        1000 training steps, linear betas 1e-4 .. 0.02 (fp32), acp = cumprod(1 - beta) (fp32), epsilon prediction,
                      skip_prk_steps False, set_alpha_to_one False (final acp = acp[0]), "leading" spacing, steps_offset 0;
                      order 1, init_noise_sigma 1, scale_model_input the identity
      set_timesteps   r = 1000 // n, ts = arange(n) r; prk = repeat(ts[-4:], 2) + tile([0, r // 2], 4), then
                      reverse(repeat(prk[:-1], 2)[1:-1]) (12 entries); plms = reverse(ts[:-3]); timesteps = prk ++ plms (n + 9)
      prev(x, t, t', m)  a = acp[t], a' = acp[t'] (acp[0] for t' < 0):
                      sqrt(a'/a) x - (a' - a) m / (a sqrt(1 - a') + sqrt(a (1 - a) a'))
      call c < 12     (Runge-Kutta) t' = t - (0 if c odd else r // 2), t0 = prk[c // 4 * 4]; c % 4 == 0: acc += e / 6, history += e,
                      cur = x; 1, 2: acc += e / 3; 3: e = acc + e / 6, acc = 0; out = prev(cur, t0, t', e)
      call c >= 12    (linear multistep) t' = t - r, history = last three + e, m = (55 e[-1] - 59 e[-2] + 37 e[-3] - 9 e[-4]) / 24,
                      out = prev(x, t, t', m)

    ``step`` is the pure-torch form (host use, any dtype; a float64 sample stays float64).  ``step_coeffs(i)`` is call i as the linear
    form ``vsys_cfg_pndm_step`` evaluates, in Python doubles from the fp32 acp."""

    order = 1
    init_noise_sigma = 1.0

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.0001, beta_end: float = 0.02,
                 beta_schedule: str = "linear", skip_prk_steps: bool = False, set_alpha_to_one: bool = False,
                 prediction_type: str = "epsilon", timestep_spacing: str = "leading", steps_offset: int = 0):
        if beta_schedule != "linear" or skip_prk_steps or set_alpha_to_one or prediction_type != "epsilon" or \
                timestep_spacing != "leading" or steps_offset != 0:
            raise NotImplementedError("PNDMScheduler: the defaults the Open-Sora-Plan v1.1 pipeline constructs it with (linear betas, "
                                      "Runge-Kutta warm-up, epsilon prediction, leading spacing, no offset) are what is built")
        self.num_train_timesteps = num_train_timesteps
        self.betas = torch.linspace(beta_start, beta_end, num_train_timesteps, dtype=torch.float32)
        self.alphas_cumprod = torch.cumprod(1.0 - self.betas, dim=0)
        self.final_alpha_cumprod = self.alphas_cumprod[0]
        self._acp = [float(v) for v in self.alphas_cumprod]
        self.num_inference_steps = None
        self.timesteps = torch.from_numpy(np.arange(0, num_train_timesteps)[::-1].copy())
        self.prk_timesteps = self.plms_timesteps = None
        self._reset()

    def _reset(self):
        self.ets: List[torch.Tensor] = []
        self.counter = 0
        self.cur_model_output = 0
        self.cur_sample = None

    def set_timesteps(self, num_inference_steps: int, device=None):
        if num_inference_steps < 4:
            raise ValueError(f"PNDMScheduler.set_timesteps({num_inference_steps}): the Runge-Kutta warm-up takes the last four of the "
                             "timesteps and the multistep the rest but three: at least 4 steps")
        self.num_inference_steps = n = int(num_inference_steps)
        r = self.num_train_timesteps // n
        ts = (np.arange(0, n) * r).round().astype(np.int64)
        prk = np.array(ts[-4:]).repeat(2) + np.tile(np.array([0, r // 2]), 4)
        self.prk_timesteps = (prk[:-1].repeat(2)[1:-1])[::-1].copy()
        self.plms_timesteps = ts[:-3][::-1].copy()
        self.timesteps = torch.from_numpy(np.concatenate([self.prk_timesteps, self.plms_timesteps]).astype(np.int64))
        self._reset()

    def scale_model_input(self, sample, *args, **kwargs):
        return sample

    def __len__(self):
        return self.num_train_timesteps

    def _transfer(self, t: int, t_prev: int) -> Tuple[float, float]:
        """prev(x, t, t', m) = A x - B m: (A, B) in Python doubles from the fp32 acp."""
        a = self._acp[t]
        ap = self._acp[t_prev] if t_prev >= 0 else self._acp[0]
        return (ap / a) ** 0.5, (ap - a) / (a * (1.0 - ap) ** 0.5 + (a * (1.0 - a) * ap) ** 0.5)

    def step_coeffs(self, i: int) -> dict:
        """Call ``i`` (0 .. n + 8) of the current ``set_timesteps`` as the linear form of vsys_cfg_pndm_step over S = (e, src0 .. src3):
        {kind, c_base, cz[5], ca[5]}.  kind "prk0" .. "prk3": src0 is the accumulator, base the sample the group started from; "prk0"
        and "plms" store e in the history, "prk0" .. "prk2" store the accumulator (``ca``).  kind "plms": src0 .. src2 are the history
        entries e[-2], e[-3], e[-4] and base the current sample."""
        n = self.num_inference_steps
        r = self.num_train_timesteps // n
        t = int(self.timesteps[i])
        cz, ca = [0.0] * 5, [0.0] * 5
        if i < len(self.prk_timesteps):
            k = i % 4
            t_prev = t - (0 if i % 2 else r // 2)
            A, B = self._transfer(int(self.prk_timesteps[i // 4 * 4]), t_prev)
            if k == 0:
                cz[0], ca[0] = -B, 1.0 / 6.0                       # the accumulator starts from zero: its buffer is not read
            elif k < 3:
                cz[0], ca[0], ca[1] = -B, 1.0 / 3.0, 1.0
            else:
                cz[0], cz[1] = -B / 6.0, -B
            return dict(kind=f"prk{k}", t=t, t_prev=t_prev, c_base=A, cz=cz, ca=ca)
        A, B = self._transfer(t, t - r)
        cz[:4] = [-B * 55.0 / 24.0, B * 59.0 / 24.0, -B * 37.0 / 24.0, B * 9.0 / 24.0]
        return dict(kind="plms", t=t, t_prev=t - r, c_base=A, cz=cz, ca=ca)

    def _get_prev_sample(self, sample, timestep, prev_timestep, model_output):
        A, B = self._transfer(int(timestep), int(prev_timestep))
        return A * sample - B * model_output

    def step(self, model_output, timestep, sample, return_dict: bool = True):
        n = self.num_inference_steps
        if n is None:
            raise ValueError("PNDMScheduler.step before set_timesteps")
        r = self.num_train_timesteps // n
        t, c = int(timestep), self.counter
        if c < len(self.prk_timesteps):
            t_prev = t - (0 if c % 2 else r // 2)
            t0 = int(self.prk_timesteps[c // 4 * 4])
            if c % 4 == 0:
                self.cur_model_output = self.cur_model_output + model_output / 6
                self.ets.append(model_output)
                self.cur_sample = sample
            elif c % 4 in (1, 2):
                self.cur_model_output = self.cur_model_output + model_output / 3
            else:
                model_output = self.cur_model_output + model_output / 6
                self.cur_model_output = 0
            prev = self._get_prev_sample(self.cur_sample, t0, t_prev, model_output)
        else:
            self.ets = self.ets[-3:]
            self.ets.append(model_output)
            e = self.ets
            m = (55 * e[-1] - 59 * e[-2] + 37 * e[-3] - 9 * e[-4]) / 24
            prev = self._get_prev_sample(sample, t, t - r, m)
        self.counter += 1
        return (prev,)


# LatteT2V constructor keywords of the published v1.1 checkpoints (LatteT2V_XL_122 with RoPE, open_sora_plan_v110_transformer_3d.py):
# 512 x 512 pixels are a 64 x 64 latent, (num_frames - 1) / 4 + 1 latent frames
def _geometry(frames_lat):
    return dict(num_layers=28, attention_head_dim=72, num_attention_heads=16, patch_size_t=1, patch_size=2, norm_type="ada_norm_single",
                caption_channels=4096, cross_attention_dim=1152, in_channels=4, out_channels=8, attention_bias=True, sample_size=(64, 64),
                video_length=frames_lat, activation_fn="gelu-approximate", norm_elementwise_affine=False, norm_eps=1e-6, use_rope=True,
                model_max_length=MAX_LENGTH)


_V110_GEOMETRY = {"65x512x512": _geometry(17), "221x512x512": _geometry(56)}


class OpenSoraPlanV110Pipeline(OpenSoraPlanPipeline):
    """The ``version == "v110"`` route of the reference's OpenSoraPlanPipeline (module docstring).  What it shares with the v1.2 pipeline
    — input checks, latent shapes, caption cleaning, the uint8 post-process, staging for ``cpu_offload`` — is inherited."""

    TEXT_VOCAB, TEXT_MAX_LENGTH = 32128, MAX_LENGTH

    def __init__(self, config: OpenSoraPlanV110Config, tokenizer=None, text_encoder=None, vae=None, transformer=None, scheduler=None,
                 device: torch.device = torch.device("cuda"), dtype: torch.dtype = torch.bfloat16):
        """pipeline_open_sora_plan.py:257-341, same parameter order.  Components left at None are read from ``config.transformer`` when
        that is a LOCAL checkpoint directory (``<transformer_type>/``, ``vae/``); ``"synthetic:<seed>"`` builds seeded weights."""
        if config.num_gpus != 1:      # before any component is read
            raise NotImplementedError(f"OpenSoraPlanV110Pipeline: num_gpus={config.num_gpus}: the v1.1 transformer has no sequence "
                                      "parallelism (open_sora_plan_v110.py)")
        self._config = config
        self._dtype = self._check_dtype(dtype)
        self._device = self._resolve_device(device, "OpenSoraPlanV110Pipeline")
        name = config.transformer
        synthetic = isinstance(name, str) and name.startswith("synthetic:")
        seed = int(name.split(":", 1)[1]) if synthetic else 1101
        if transformer is None or is_foreign_module(transformer, LatteT2V):
            file_cfg, sd = module_state(transformer) if transformer is not None else read_component(name, config.transformer_type)
            tcfg = dict(_V110_GEOMETRY[config.transformer_type])
            tcfg.update(ctor_kwargs(LatteT2V.__init__, file_cfg))
            tcfg.update(config.transformer_config or {})
            transformer = LatteT2V(**tcfg, device=self._device)
            if sd is None:
                c = transformer.config
                sd = synth_state_dict(num_layers=c.num_layers, num_heads=c.num_attention_heads, caption_channels=c.caption_channels,
                                      in_channels=c.in_channels, out_channels=c.out_channels, patch_size=c.patch_size, seed=seed)
            transformer.load_state_dict(sd)
        self.transformer = transformer
        if transformer.config.out_channels != 2 * transformer.config.in_channels:
            raise NotImplementedError("OpenSoraPlanV110Pipeline: the step kernel drops a learned-sigma half (out_channels = 2 in_channels)")
        self.transformer.force_images = False
        if scheduler is None:
            scheduler = PNDMScheduler()
        self.scheduler = self._check_scheduler(scheduler, "step_coeffs", "videosys_amd.pipeline_open_sora_plan_v110.PNDMScheduler")
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
        self.text_encoder = self._build_text_encoder(text_encoder, tokenizer)      # T5 v1.1 at 300 tokens (TEXT_VOCAB, TEXT_MAX_LENGTH)
        pab.set_pab_manager(config.pab_config if config.enable_pab else None)
        self._steps = program.StepCache()   # (geometry, text length) -> (Program, pred)
        self._step_bufs = None
        self.pab_trace: List[list] = []     # PAB on: per model call of the last generate(), every block's (attention, cross, mlp) decision
        self._set_parallel()
        self._init_stages(config.cpu_offload, self._device, text_encoder=getattr(self.text_encoder, "encoder", None),
                          transformer=self.transformer, vae=getattr(self.vae, "vae", None))

    def _vae_from_state(self, sd):
        from .vae_open_sora_plan_v110 import CausalVAEModelWrapper

        return CausalVAEModelWrapper(sd, device=self._device, **(self._config.vae_config or {}))

    def _load_vae(self, name, synthetic_seed):
        """:288 CausalVAEModelWrapper(config.transformer, subfolder="vae"): a local ``vae/`` directory, or seeded weights for
        ``"synthetic:<seed>"``; None when neither is there (generate() then returns latents)."""
        from .vae_open_sora_plan_v110 import CausalVAEModelWrapper

        if synthetic_seed is not None:
            return CausalVAEModelWrapper(f"synthetic:{synthetic_seed}", device=self._device, **(self._config.vae_config or {}))
        if not isinstance(name, str):
            return None
        sd = read_component(name, "vae")[1]
        return self._vae_from_state(sd) if sd is not None else None

    def _set_parallel(self, dp_size: Optional[int] = None, sp_size: Optional[int] = None, enable_cp: Optional[bool] = False,
                      parallel_mgr=None):
        """:349-363 on one rank: the transformer refuses more (open_sora_plan_v110.LatteT2V.enable_parallel)."""
        self._steps.clear()
        self.transformer.enable_parallel(dp_size or 1, sp_size or 1, enable_cp, parallel_mgr=parallel_mgr)

    def _decode_group(self):
        return None                          # one rank: the plain decode

    def check_inputs(self, prompt, height, width, negative_prompt, callback_steps, prompt_embeds=None, negative_prompt_embeds=None,
                     prompt_attention_mask=None, negative_prompt_attention_mask=None):
        """:693-752.  The v1.1 route has no use for the two masks (:1051-1052), so embeddings may be handed in without them (the
        reference's check would fail on the missing masks' ``.shape``); masks that are given are checked as the reference does."""
        if prompt_attention_mask is None or negative_prompt_attention_mask is None:
            prompt_attention_mask = negative_prompt_attention_mask = torch.empty(0)
        super().check_inputs(prompt, height, width, negative_prompt, callback_steps, prompt_embeds, negative_prompt_embeds,
                             prompt_attention_mask, negative_prompt_attention_mask)

    # ------------------------------------------------------------------------------------------------ text side
    def encode_prompt(self, prompt, do_classifier_free_guidance: bool = True, negative_prompt: str = "", num_images_per_prompt: int = 1,
                      device=None, prompt_embeds: Optional[torch.Tensor] = None, negative_prompt_embeds: Optional[torch.Tensor] = None,
                      clean_caption: bool = False, mask_feature: bool = True):
        """:375-536 -> (prompt_embeds [B, L', d], negative_prompt_embeds or None).  Prompts are encoded at 300 tokens, the negative
        prompt once per prompt at the same length.  With ``mask_feature``, embeddings ENCODED here are masked (:517-533): a batch of one
        is cut to its token count ``keep_index = mask.sum()`` and the negative embeddings are sliced to the same length, pad-position
        outputs included; a batch of several keeps all 300 positions with the prompt embeddings multiplied by the mask (the negative
        ones untouched).  Embeddings passed in are not masked.  No mask is returned: none reaches the transformer."""
        device = device or self._device
        if prompt is not None and isinstance(prompt, str):
            batch_size = 1
        elif prompt is not None and isinstance(prompt, list):
            batch_size = len(prompt)
        else:
            batch_size = prompt_embeds.shape[0]
        mask = None
        if prompt_embeds is None:
            prompt_embeds, mask = self._encode(self._text_preprocessing(prompt, clean_caption), MAX_LENGTH)
        prompt_embeds = prompt_embeds.to(dtype=self._dtype, device=device)
        bs_embed, seq_len, _ = prompt_embeds.shape
        prompt_embeds = prompt_embeds.repeat(1, num_images_per_prompt, 1).view(bs_embed * num_images_per_prompt, seq_len, -1)
        if mask is not None:
            mask = mask.to(device).view(bs_embed, -1).repeat(num_images_per_prompt, 1)
        if do_classifier_free_guidance and negative_prompt_embeds is None:
            uncond = self._text_preprocessing([negative_prompt] * batch_size, clean_caption)
            negative_prompt_embeds, _ = self._encode(uncond, prompt_embeds.shape[1])
        if do_classifier_free_guidance:
            seq_len = negative_prompt_embeds.shape[1]
            negative_prompt_embeds = negative_prompt_embeds.to(dtype=self._dtype, device=device)
            negative_prompt_embeds = negative_prompt_embeds.repeat(1, num_images_per_prompt, 1).view(batch_size * num_images_per_prompt, seq_len, -1)
        else:
            negative_prompt_embeds = None
        if mask_feature and mask is not None:
            masked, keep = self.mask_text_embeddings(prompt_embeds.unsqueeze(1), mask)
            prompt_embeds = masked.squeeze(1)
            if negative_prompt_embeds is not None:
                negative_prompt_embeds = negative_prompt_embeds[:, :keep, :]
        return prompt_embeds, negative_prompt_embeds

    # ------------------------------------------------------------------------------------------------ denoise step
    def _model(self, xin, t, enc, all_ts, temporal=True):
        nb = xin.shape[0]
        return self.transformer(xin, timestep=torch.full((nb,), int(t), dtype=torch.int64), all_timesteps=all_ts, encoder_hidden_states=enc,
                                encoder_attention_mask=None, added_cond_kwargs={"resolution": None, "aspect_ratio": None},
                                enable_temporal_attentions=temporal, return_dict=False)[0]

    def _pab_pattern(self, t_int, all_ts):
        """The decisions the model's blocks will make at this call, block by block in execution order (spatial, temporal, spatial,
        ...), WITHOUT touching the blocks' state: (attention broadcast?, cross broadcast? — None for a temporal block —, MLP
        broadcast?).  They are functions of the timestep and the blocks' counters (pab.py), which is what the blocks consult."""
        mgr = pab.PAB_MANAGER
        ats = [int(v) for v in torch.as_tensor(all_ts).tolist()]
        out = []
        for st in self.transformer.states:
            attn = (mgr.if_broadcast_temporal if st.temporal else mgr.if_broadcast_spatial)(t_int, st.attn_count)[0]
            cross = None if st.temporal else mgr.if_broadcast_cross(t_int, st.cross_count)[0]
            out.append((attn, cross, mgr.if_skip_mlp(t_int, st.mlp_count, st.block_idx, ats, st.temporal)[0]))
        return out

    def _prepare_text(self, enc):
        """The text K / V of every block are step-invariant: made resident here, eagerly (a no-op for the text they were made for),
        so that the recorded step does not contain the caption projection and the 2 x depth K / V launches and a replay does not
        repeat them.  ``enc`` [2B, 1, L, d]: the transformer caches by the tensor it is handed, ``enc[:, 0]`` (latte.py)."""
        self.transformer._encode_text(enc[:, 0], None, 0)

    def _issue_model(self, xin, t, enc, all_ts, temporal=True):
        """One CFG model call -> fp32 [2B, 2C, T, h, w]: through the launch program recorded for this (geometry, text length), or
        eagerly with PAB on or with ``transformer.use_programs`` False."""
        tr = self.transformer
        if pab.enable_pab():
            self.pab_trace.append(self._pab_pattern(int(t), all_ts))
        if pab.enable_pab() or not temporal or not getattr(tr, "use_programs", True):
            return self._steps.eager(lambda: self._model(xin, t, enc, all_ts, temporal))
        key = (tuple(xin.shape), tuple(enc.shape))
        if key not in self._steps:
            self._prepare_text(enc)                               # outside the recording
        # (on a hit) the one per-step input besides the latents
        return self._steps.run(key, lambda: self._model(xin, t, enc, all_ts), lambda pred: tr.step_timesteps(xin.shape[0]).fill_(float(t)))

    def _buffers(self, z0, enc):
        """Resident operands of a call — the two fp32 latent buffers the warm-up ping-pongs between, the ring of four history slots,
        the Runge-Kutta accumulator, the model input as the step kernel leaves it (bf16 [2B, ...]) and as the patch embedding reads it
        (fp32), the text — kept across generate() calls of one geometry so that the recorded program (which holds the addresses of
        ``xin``) stays valid.  The recorded step reads the resident text K / V that ``_prepare_text`` made for THIS text (the
        transformer allocates new ones for a new text), so a new prompt drops the programs."""
        b = self._step_bufs
        if b is not None and b["z"][0].shape == z0.shape and b["enc"].shape == enc.shape:
            if not torch.equal(b["enc"], enc):
                self._steps.clear()
                b["enc"].copy_(enc)
            b["z"][0].copy_(z0)
            return b
        self._steps.clear()
        z = z0.to(device=self._device, dtype=torch.float32).contiguous().clone()
        new = lambda: torch.empty_like(z)
        two = (2 * z.shape[0],) + tuple(z.shape[1:])
        self._step_bufs = dict(z=[z, new()], hist=[new() for _ in range(4)], acc=new(),
                               model_in=torch.empty(two, dtype=torch.bfloat16, device=self._device),
                               xin=torch.empty(two, dtype=torch.float32, device=self._device), enc=enc.contiguous().clone())
        return self._step_bufs

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
        """pipeline_open_sora_plan.py:911-1182 at ``version == "v110"`` with the reference's parameters and defaults (module docstring for
        the sampler): ``num_inference_steps`` + 9 model calls.  ``output_type="latents"`` returns the fp32 latents (also what comes back
        when no VAE is attached); anything else the uint8 video [B, num_frames, height, width, 3] on the CPU.  ``eta`` is ignored as the
        reference's scheduler ignores it; ``max_sequence_length`` and the two attention masks are accepted and unused (:1051-1052: v1.1
        encodes at 300 tokens and hands the transformer no mask)."""
        if isinstance(generator, (list, tuple)):
            raise NotImplementedError("a list of generators: the start latents are drawn from one generator")
        tc = self.transformer.config
        ss = tc.sample_size_hw
        height, width = ss[0] * self.vae_scale_factor[1], ss[1] * self.vae_scale_factor[2]
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
        prompt_embeds, negative_prompt_embeds = self.encode_prompt(
            prompt, do_cfg, negative_prompt=negative_prompt, num_images_per_prompt=num_images_per_prompt, device=self._device,
            prompt_embeds=prompt_embeds, negative_prompt_embeds=negative_prompt_embeds, clean_caption=clean_caption, mask_feature=mask_feature)
        enc = torch.cat([negative_prompt_embeds if do_cfg else prompt_embeds, prompt_embeds], dim=0)[:, None]   # (:1072-1073, :1127-1128)
        sch = self.scheduler
        sch.set_timesteps(num_inference_steps, device=self._device)                                              # (:1079-1080)
        timesteps = sch.timesteps
        self._enter_stage("transformer")
        self.transformer.reset_pab_state()
        self.pab_trace = []
        if generator is None:
            generator = torch.Generator(device=self._device).manual_seed(seed)
        z0 = self.prepare_latents(batch_size * num_images_per_prompt, tc.in_channels, num_frames, height, width, torch.float32,
                                  self._device, generator, latents)
        b = self._buffers(z0, enc)
        (cur, other), hist, acc, model_in, xin, enc = b["z"], b["hist"], b["acc"], b["model_in"], b["xin"], b["enc"]
        self._prepare_text(enc)                                             # step-invariant: once per prompt, never inside a recorded step
        model_in.copy_(cur.to(torch.bfloat16).repeat(2, 1, 1, 1, 1))        # scale_model_input is the identity (:1109-1110)
        g = guidance_scale if do_cfg else 1.0
        n_hist = 0
        for i, t in progress_wrap(list(enumerate(timesteps.tolist())), verbose):
            xin.copy_(model_in)
            pred = self._issue_model(xin, t, enc, timesteps, enable_temporal_attentions)
            k = sch.step_coeffs(i)
            kind = k["kind"]
            e_out = None
            if kind in ("prk0", "plms"):
                e_out = hist[n_hist % 4]
                n_hist += 1
            if kind == "plms":                       # in place; the three entries before this call's, newest first
                srcs = [hist[(n_hist - 1 - j) % 4] for j in (1, 2, 3)]
                vops.cfg_pndm_step(pred, model_in, cur, g, k["c_base"], k["cz"], None, base=cur, srcs=srcs, e_out=e_out)
            else:                                    # ``cur`` is the scheduler's cur_sample: read, never written, until the group ends
                vops.cfg_pndm_step(pred, model_in, other, g, k["c_base"], k["cz"], k["ca"], base=cur, srcs=(acc,), e_out=e_out,
                                   aux_out=None if kind == "prk3" else acc)
                if kind == "prk3":
                    cur, other = other, cur
            if callback is not None and i % callback_steps == 0:                                                 # (:1164-1167), 9 warm-up calls
                if i == len(timesteps) - 1 or (i + 1) > len(timesteps) - num_inference_steps * sch.order:
                    callback(i, t, other if kind in ("prk0", "prk1", "prk2") else cur)
        b["z"] = [cur, other]
        dsp.check_exchange(self.transformer)
        if self.vae is None or output_type in ("latent", "latents"):
            return self._leave(cur.clone(), return_dict)
        self._enter_stage("vae")
        return self._leave(self.decode_latents(cur)[:, :num_frames, :height, :width], return_dict)
