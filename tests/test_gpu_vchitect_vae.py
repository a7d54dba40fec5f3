"""-m gpu: the SD3 VAE decode of the Vchitect-2.0 pipeline (videosys_amd/vae_sd3.py, csrc/vae_sd3.hip).

Kernels, bit for bit against torch / numpy restatements of their roundings on the CPU:
  * vsys_vae_first_im2col_nc: bf16(bf16(bf16(z) / scaling) + shift), every step an explicit fp32 operation rounded once (a true fp32
    division), column tap * Cz + c, zero at the image border and in the pad columns;
  * vsys_pixels_to_u8: d = clamp(bf16(bf16(x / 2) + 0.5), 0, 1), byte = numpy.round(float32(d) * 255) (half to even), on a grid with a
    zero border whose rows, and whose channels from 3 on, hold values that would show in the result.

Decoder, F = 2 frames of a 6 x 10 latent (60 tokens: the 128-row pad path of the mid attention) on synthetic weights against
oracle.vae_oracle.spatial_decode run in float64 on the bf16-rounded weights (identity 16 x 16 post_quant_conv, decoder keys re-prefixed).
Bound (the project's, tests/test_gpu_vchitect_model.py): the same oracle in bf16 on the CPU against its float64 self is the floor; the
HIP decoder's RMS error against float64 must stay within 1.5 x that floor.  decode_u8 must equal the restated post-process of decode's
own bf16 output exactly."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SF, SH = 1.5305, 0.0609


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def scale_shift_bf16(z):
    """`latents / scaling_factor + shift_factor` on bf16 latents: three roundings, fp32 arithmetic in between."""
    zb = z.to(torch.bfloat16)
    a = (zb.float() / torch.tensor(SF, dtype=torch.float32)).to(torch.bfloat16)
    return (a.float() + torch.tensor(SH, dtype=torch.float32)).to(torch.bfloat16)


def im2col_ref(z, kcols):
    F, Cz, H, W = z.shape
    v = scale_shift_bf16(z)
    out = torch.zeros(F, H, W, kcols, dtype=torch.bfloat16)
    for dy in range(3):
        for dx in range(3):
            tap = 3 * dy + dx
            for h in range(H):
                for w in range(W):
                    hh, ww = h + dy - 1, w + dx - 1
                    if 0 <= hh < H and 0 <= ww < W:
                        out[:, h, w, tap * Cz:(tap + 1) * Cz] = v[:, :, hh, ww]
    return out.reshape(F * H * W, kcols)


@pytest.mark.parametrize("Cz,kcols", [(16, 160), (5, 64)])
def test_first_im2col_nc_bit_exact(Cz, kcols):
    from videosys_amd import vchitect_ops as vops

    F, H, W = 2, 3, 5
    g = torch.Generator().manual_seed(Cz)
    z = torch.randn(F, Cz, H, W, generator=g) * 2.0            # fp32 values that are NOT bf16-exact: the first rounding counts
    z[0, 0, 0, 0], z[1, Cz - 1, H - 1, W - 1] = 0.0, -3.0e-3
    got = vops.vae_first_im2col_nc(z.to(dev()).contiguous(), kcols, SF, SH).cpu()
    want = im2col_ref(z, kcols)
    assert got.shape == want.shape == (F * H * W, kcols)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert float(got[:, 9 * Cz:].abs().max()) == 0.0                                       # pad columns
    rows = got.view(F, H, W, kcols)
    assert float(rows[:, 0, :, :3 * Cz].abs().max()) == 0.0 and float(rows[:, H - 1, :, 6 * Cz:9 * Cz].abs().max()) == 0.0   # dy = 0 / 2 rows
    left, right = [t * Cz + c for t in (0, 3, 6) for c in range(Cz)], [t * Cz + c for t in (2, 5, 8) for c in range(Cz)]
    assert float(rows[:, :, 0, left].abs().max()) == 0.0 and float(rows[:, :, W - 1, right].abs().max()) == 0.0
    assert float(rows[:, 1, 1, :9 * Cz].abs().min()) > 0.0                                # an inner pixel has all 9 taps
    # shift alone (z = 0) must come out as bf16(shift): the border zero is a PADDING zero, not a latent zero
    assert float(rows[0, 0, 0, 4 * Cz]) == float(torch.tensor(SH).to(torch.bfloat16))


def u8_ref(x):
    """VaeImageProcessor.postprocess(image, "pil") on bf16 pixels [..., 3] -> uint8, the denormalize on the bf16 tensor."""
    d = ((x.float() / 2).to(torch.bfloat16).float() + 0.5).to(torch.bfloat16).clamp(0, 1)
    return torch.from_numpy(np.round(d.float().numpy() * 255).astype(np.uint8))


def test_pixels_to_u8_bit_exact():
    from videosys_amd import vchitect_ops as vops
    from videosys_amd.ops import VaeGrid

    N, H, W, ldx, Ftot, f0 = 2, 4, 6, 128, 4, 1
    g = VaeGrid(N, 1, H, W, 1, 0)
    gen = torch.Generator().manual_seed(3)
    pix = (torch.rand(N, H, W, 3, generator=gen) * 3.0 - 1.5).to(torch.bfloat16)
    special = torch.tensor([-2.0, -1.0, -1.00390625, 0.0, 1.0, 1.0078125, 2.0, -0.0, 0.99609375, -0.99609375, 3.0e-3, 0.5, -0.5],
                           dtype=torch.bfloat16)            # below -1, above 1, x = 0 -> d = 0.5 -> 127.5, the only exact half-way byte
    pix.view(-1)[:special.numel()] = special
    want_px = u8_ref(pix)
    assert int(want_px.view(-1)[3]) == 128 and int(want_px.min()) == 0 and int(want_px.max()) == 255
    x = torch.full((g.rows, ldx), 7.0, dtype=torch.bfloat16)          # border rows and channels >= 3 would read as byte 255
    x.view(N, H + 2, W + 2, ldx)[:, 1:-1, 1:-1, :3] = pix
    out = torch.full((Ftot, H, W, 3), 77, dtype=torch.uint8, device=dev())
    vops.pixels_to_u8(x.to(dev()), g, out, f0)
    out = out.cpu()
    assert torch.equal(out[f0:f0 + N], want_px)
    assert bool((out[:f0] == 77).all()) and bool((out[f0 + N:] == 77).all())            # frames outside [f0, f0 + N) are the caller's


_DEC = {}


def decoder_case():
    """(decoder, latents fp32 [F, 16, 6, 10] bf16-exact, float64 oracle [F, 3, 48, 80], bf16 floor) — computed once."""
    if not _DEC:
        from oracle import vae_oracle as O
        from videosys_amd import vae_sd3

        sd = vae_sd3.synth_state_dict(5)
        osd = {"spatial_vae.module." + k: v for k, v in sd.items()}
        osd["spatial_vae.module.post_quant_conv.weight"] = torch.eye(16).reshape(16, 16, 1, 1)
        osd["spatial_vae.module.post_quant_conv.bias"] = torch.zeros(16)
        z = torch.randn(2, 16, 6, 10, generator=torch.Generator().manual_seed(9)).to(torch.bfloat16).float()
        with torch.no_grad():
            want = O.spatial_decode({k: v.double() for k, v in osd.items()}, z.double())
            low = O.spatial_decode({k: v.to(torch.bfloat16) for k, v in osd.items()}, z.to(torch.bfloat16))
        floor = float((low.double() - want).pow(2).mean().sqrt())
        _DEC["case"] = (vae_sd3.AutoencoderKLSD3Decoder(sd, device=dev()), z, want, floor)
    return _DEC["case"]


def test_decoder_within_the_bf16_floor():
    dec, z, want, floor = decoder_case()
    c = dec.config
    assert (c.latent_channels, tuple(c.block_out_channels), c.scaling_factor, c.shift_factor) == (16, (128, 256, 512, 512), 1.5305, 0.0609)
    out = dec.decode(z.to(dev()), return_dict=False)
    assert isinstance(out, tuple) and out[0].shape == (2, 3, 48, 80) and out[0].dtype == torch.bfloat16
    got = out[0].float().cpu()
    err = float((got.double() - want).pow(2).mean().sqrt())
    print(f"[sd3 decoder] HIP rms error {err:.4e}, bf16 floor {floor:.4e}, ratio {err / floor:.3f}, output rms {float(want.pow(2).mean().sqrt()):.3f}")
    assert torch.isfinite(got).all()
    assert err <= 1.5 * floor, f"SD3 decoder: HIP rms error {err:.4e} vs float64 > 1.5 x bf16 floor {floor:.4e}"
    # frames are independent: one frame per launch gives the same bits as two
    dec.frames_per_launch, keep = 1, dec.frames_per_launch
    try:
        assert torch.equal(dec.decode(z.to(dev()))[0], out[0])
    finally:
        dec.frames_per_launch = keep


def test_decode_u8_equals_the_postprocess_of_decode():
    dec, z, _, _ = decoder_case()
    lat = (z * 1.3 + 0.2).contiguous()                                   # sampler-side latents (fp32, not bf16-exact)
    u8 = dec.decode_u8(lat[None].to(dev()))
    assert u8.shape == (2, 48, 80, 3) and u8.dtype == torch.uint8 and u8.is_cuda
    img = dec.decode(scale_shift_bf16(lat).to(dev()))[0]                 # [F, 3, H, W] bf16: what decode_u8 post-processes inside
    assert torch.equal(u8.cpu(), u8_ref(img.cpu().permute(0, 2, 3, 1)))
    assert 0 < float(u8.float().std())                                   # not a constant image
    with pytest.raises(ValueError):
        dec.decode_u8(lat.to(dev()))
