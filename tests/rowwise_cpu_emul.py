"""TEST INFRASTRUCTURE: plain restatements of the row-wise kernels' arithmetic (csrc/rowwise.hip, csrc/t5_ops.hip) in torch fp32 on the CPU,
with the bf16 roundings where the kernels have them, behind the signatures of videosys_amd.ops / vchitect_ops — so a case of
tests/rowwise_numerics_cases.py calls them exactly as it calls the HIP wrappers.  ``Emul(defect)`` plants one defect (the names are the
keys of CAUGHT_BY in tests/test_numerics_rowwise_cpu.py); ``Emul(variant)`` with a name from VARIANTS rounds once fewer than the contract.

Vectors that the wrappers take as a pointer to sample 0 plus a sample stride arrive here as 2-D views [samples, C]."""
import math

import torch

BF = torch.bfloat16
VARIANTS = ("final_fp32_activation", "patch_latent_unrounded", "skinny_res_one_rounding")


def bfr(t):
    """Round fp32 to bf16 and widen again (bf2f(f2bf(.)))."""
    return t.to(BF).float()


def _seq_sum(t):
    """An fp32 sum taken strictly in order (one accumulator), [rows, C] -> [rows, 1]."""
    s = torch.zeros(t.shape[0], dtype=torch.float32)
    for j in range(t.shape[1]):          # (torch.cumsum accumulates in double on the CPU)
        s = s + t[:, j]
    return s[:, None]


class Emul:
    def __init__(self, defect=None):
        self.defect = defect

    # ---------------------------------------------------------------- statistics
    def _stats(self, x, eps, rms=False):
        """(mean, rstd) [rows, 1] fp32: two passes over the row, as the kernels take them."""
        d = self.defect
        C = x.shape[1]
        div = float(C)
        if d == "padded_width":
            div = float(-(-C // 512) * 512)          # the 64 lanes x 8 elements x MAXV registers of the row
        if d == "eps_swapped":
            eps = 1e-5 if eps < 5e-6 else 1e-6
        if d == "no_eps":
            eps = 0.0
        if d == "one_pass" and not rms:
            mean = _seq_sum(x) / div
            var = (_seq_sum(x * x) / div - mean * mean).clamp_min(0.0)
            return mean, torch.rsqrt(var + eps)
        mean = torch.zeros(x.shape[0], 1) if (rms and d != "rms_minus_mean") else x.sum(dim=1, keepdim=True) / div
        dd = x - mean
        q = (dd * dd).sum(dim=1, keepdim=True)
        var = q / (div - 1.0) if d == "var_c_minus_1" else q / div
        return mean, torch.rsqrt(var + eps)

    def _sample(self, rows, rps):
        r = torch.arange(rows)
        if self.defect == "sample_rps_plus_1":
            return r // (rps + 1)
        if self.defect == "sample_0":
            return torch.zeros_like(r)
        return r // rps

    # ---------------------------------------------------------------- LayerNorm + modulate
    def adaln_modulate(self, x, shift, scale, rows_per_sample, mod_stride, eps=1e-6, out=None):
        x = x.float()
        rows, C = x.shape
        mean, rstd = self._stats(x, eps)
        if self.defect == "tail_stats" and 1024 < C <= 1536 and rows_per_sample % 2 == 0:     # the two-rows-per-wave kernel
            odd = torch.arange(rows) % 2 == 1
            src = torch.arange(rows) - odd.long()
            mean, rstd = mean[src], rstd[src]
        b = self._sample(rows, rows_per_sample).clamp_max(shift.shape[0] - 1)
        a, m = shift.float()[b], scale.float()[b]
        if self.defect == "shift_scale_swapped":
            a, m = m, a
        return ((x - mean) * rstd * (1.0 + m) + a).to(BF)

    def ln_modulate(self, x, ln_w, ln_b, shift, scale, rows_per_sample, mod_stride=0, seg_split=0, mod_alt=0, eps=1e-5, out=None):
        x = x.float()
        rows, C = x.shape
        mean, rstd = self._stats(x, eps)
        o = (x - mean) * rstd
        if ln_w is not None:
            o = o * ln_w.float() + ln_b.float()
        if shift is not None:
            b = self._sample(rows, rows_per_sample).clamp_max(shift.shape[0] - 1)
            pos = torch.arange(rows) - (torch.arange(rows) // rows_per_sample) * rows_per_sample
            text = (pos <= seg_split) if self.defect == "seg_split_off_by_one" else (pos < seg_split)
            text = (text & (seg_split > 0))[:, None]
            # the vectors ``mod_alt`` elements further on in the same sample's row of the modulation buffer
            alt = lambda v: torch.as_strided(v, v.shape, v.stride(), v.storage_offset() + mod_alt)
            a = torch.where(text, alt(shift).float()[b], shift.float()[b])
            m = torch.where(text, alt(scale).float()[b], scale.float()[b])
            if self.defect == "shift_scale_swapped":
                a, m = m, a
            o = o * (1.0 + m) + a
        return o.to(BF)

    def gate_add_rows(self, x, y, gate, rows_per_sample, gate_stride, seg_split=0, gate_alt=0):
        rows = x.shape[0]
        b = torch.arange(rows) // rows_per_sample
        pos = torch.arange(rows) - b * rows_per_sample
        text = ((pos < seg_split) & (seg_split > 0))[:, None]
        alt = torch.as_strided(gate, gate.shape, gate.stride(), gate.storage_offset() + gate_alt)
        g = torch.where(text, alt.float()[b], gate.float()[b])
        return (x.float() + bfr(g * y.float())).to(BF)

    # ---------------------------------------------------------------- final layer
    def _final_tokens(self, x, table, tvec, w, bias, rows_per_sample, eps):
        x = x.float()
        rows, C = x.shape
        mean, rstd = self._stats(x, eps)
        b = torch.arange(rows) // rows_per_sample
        t = tvec.float()[b]
        shift = bfr(table.float()[1 if self.defect == "final_scale_row_for_shift" else 0] + t)
        scale = bfr(table.float()[1] + t)
        a = (x - mean) * rstd * (1.0 + scale) + shift
        if self.defect != "final_fp32_activation":
            a = bfr(a)
        wf = w.float()
        if self.defect == "final_bf16_partials":       # the accumulator (seeded with the bias) rounded to bf16 after every 64 terms
            accum = bias.float()[None].expand(rows, -1)
            for c0 in range(0, C, 64):
                accum = bfr(accum + a[:, c0:c0 + 64] @ wf[:, c0:c0 + 64].t())
            return accum
        return bfr(a @ wf.t() + bias.float())

    def final_layer(self, x, table, tvec, w, bias, B, T, Hp, Wp, H, W, patch, Cout, eps=1e-6):
        tok = self._final_tokens(x, table, tvec, w, bias, T * Hp * Wp, eps)
        v = tok.reshape(B, T, Hp, Wp, patch[1], patch[2], Cout).permute(0, 6, 1, 2, 4, 3, 5).reshape(B, Cout, T, Hp * patch[1], Wp * patch[2])
        return v[:, :, :, :H, :W].contiguous()

    def final_layer_tokens(self, x, table, tvec, w, bias, B, T, Sl, eps=1e-6):
        return self._final_tokens(x, table, tvec, w, bias, T * Sl, eps).reshape(B, T, Sl, -1)

    def unpatchify_tokens(self, tokens, P, B, T, Sl, Hp, Wp, H, W, patch, Cout):
        seq = tokens.permute(1, 2, 0, 3, 4).reshape(B, T, P * Sl, -1)[:, :, :Hp * Wp]
        v = seq.reshape(B, T, Hp, Wp, patch[1], patch[2], Cout).permute(0, 6, 1, 2, 4, 3, 5).reshape(B, Cout, T, Hp * patch[1], Wp * patch[2])
        return v[:, :, :, :H, :W].contiguous()

    # ---------------------------------------------------------------- patch embed
    def patch_embed(self, z, w, bias, pos, B, patch, C):
        import torch.nn.functional as F

        Bz, Cin, T, H, W = z.shape
        ph, pw = patch[1], patch[2]
        x = z if self.defect == "patch_latent_unrounded" else bfr(z)
        padding = (0, (-W) % pw, 0, (-H) % ph)
        if self.defect == "patch_pad_is_edge":
            x = F.pad(x.reshape(Bz * Cin, T, H, W), padding, mode="replicate").reshape(Bz, Cin, T, H + padding[3], W + padding[1])
        else:
            x = F.pad(x, padding)
        b = torch.arange(B)
        x = x[b.clamp_max(Bz - 1) if self.defect == "patch_b_clamped" else b % Bz]
        v = F.conv3d(x, w.float(), bias.float(), stride=(1, ph, pw))              # [B, C, T, Hp, Wp]
        v = bfr(v).flatten(3).permute(0, 2, 3, 1)                                 # [B, T, S, C]
        return (v + pos.float()).to(BF)

    def patch_embed_shard(self, z, w, bias, pos, B, patch, C, s0, Sl):
        full = self.patch_embed(z, w, bias, pos, B, patch, C)
        S = full.shape[2]
        out = torch.zeros(B, full.shape[1], Sl, C, dtype=BF)
        n = max(0, min(S, s0 + Sl) - s0)
        out[:, :, :n] = full[:, :, s0:s0 + n]
        return out

    # ---------------------------------------------------------------- T5 pieces
    def rms_norm_rows(self, x, w, eps=1e-6, out=None):
        x = x.float()
        mean, rstd = self._stats(x, eps, rms=True)
        return (w.float() * bfr((x - mean) * rstd)).to(BF)

    def geglu(self, h, out=None):
        F_ = h.shape[1] // 2
        a, b = h.float()[:, :F_], h.float()[:, F_:]
        if self.defect == "geglu_erf":
            g = torch.nn.functional.gelu(a)
        else:
            u = 0.7978845608028654 * a * (1.0 + 0.044715 * a * a)
            g = a / (1.0 + torch.exp(-2.0 * u))
        return (bfr(g) * b).to(BF)

    def linear_skinny(self, x, M, w, res=None, out=None, nsplit=None, part=None, wide=None):
        K = x.shape[1]
        Ks = -(-(K // 32) // nsplit) * 32
        p = sum(x[:M, k0:k0 + Ks].float() @ w[:, k0:k0 + Ks].float().t() for k0 in range(0, K, Ks))
        if res is None:
            return p.to(BF)
        return ((p if self.defect == "skinny_res_one_rounding" else bfr(p)) + res[:M].float()).to(BF)

    # ---------------------------------------------------------------- embeddings and scheduler steps
    def timestep_embedding(self, t, dim=256):
        half = dim // 2
        k = torch.arange(half, dtype=torch.float32)
        den = float(half - 1) if self.defect == "ts_half_minus_1" else float(half)
        f = torch.exp(torch.tensor(-9.210340371976184, dtype=torch.float32) * k / den)
        a = t[:, None] * f[None]
        parts = [torch.sin(a), torch.cos(a)] if self.defect == "ts_halves_swapped" else [torch.cos(a), torch.sin(a)]
        return torch.cat(parts, dim=1).to(BF)

    def cfg_euler_step(self, z, model_out, guidance, dt):
        return self.cfg_linear_step(z, model_out, guidance, 1.0, dt, cond_first=True)

    def cfg_linear_step(self, z, model_out, guidance, c_z, c_eps, cond_first=False):
        Bz, Cin = z.shape[:2]
        if self.defect == "cfg_cond_first_inverted":
            cond_first = not cond_first
        h0, h1 = model_out[:Bz, :Cin], model_out[Bz:, :Cin]
        cond, unc = (h0, h1) if cond_first else (h1, h0)
        f = lambda v: torch.tensor(v, dtype=torch.float32)
        return f(c_z) * z + f(c_eps) * (unc + f(guidance) * (cond - unc))
