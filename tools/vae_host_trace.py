"""Host-side fingerprint of the five VAE modules: for a fixed list of small decodes / encodes on synthetic weights, the sha256 of the
output bytes and the sha256 of the LAUNCH TRACE — every ``ops._call`` in order: the entry point's name and every argument that is not
a device address (``_lib.SIGNATURES`` tells the kinds apart; a grid descriptor is recorded as its six int64 values).  Run on two
trees, equal hashes mean: the same launches with the same integer / float arguments, fed the same weights.  An unequal output hash
under an equal trace hash is a weight built differently; an unequal trace hash is a changed launch.

    python tools/vae_host_trace.py [--out FILE]        (GPU)   cases + synthetic weights
    python tools/vae_host_trace.py --cpu [--out FILE]          sha256 of every module's synth_state_dict (key order + bytes) only

Prints one JSON object (and writes it to --out)."""
import argparse
import ctypes
import hashlib
import json
import os
import struct
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")


def sd_hash(sd) -> str:
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(str(tuple(v.shape)).encode())
        h.update(v.contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def tensor_hash(t: torch.Tensor) -> str:
    t = t.detach().cpu().contiguous()
    return hashlib.sha256(str((t.dtype, tuple(t.shape))).encode() + t.view(torch.uint8).numpy().tobytes()).hexdigest()


def synth_hashes() -> dict:
    from videosys_amd import vae_cogvideox, vae_open_sora, vae_open_sora_plan, vae_sd3, vae_svd_temporal

    out = {}
    for seed in (0, 3, 7):
        out[f"open_sora:{seed}"] = sd_hash(vae_open_sora.synth_state_dict(seed))
    out["open_sora:7:encoder"] = sd_hash(vae_open_sora.synth_state_dict(7, encoder=True))
    for seed in (5, 7):
        out[f"svd_temporal:{seed}"] = sd_hash(vae_svd_temporal.synth_state_dict(seed))
    for seed in (3, 5):
        out[f"sd3:{seed}"] = sd_hash(vae_sd3.synth_state_dict(seed))
    for seed in (5, 13):
        out[f"cogvideox:{seed}"] = sd_hash(vae_cogvideox.synth_state_dict(seed))
    for hs in (32, 128):
        out[f"open_sora_plan:1203:{hs}"] = sd_hash(vae_open_sora_plan.synth_state_dict(1203, hs))
    return out


class Trace:
    """Replaces ``_call`` in ops and in the modules that imported it by name; ``digest()`` empties the log."""

    def __init__(self):
        from videosys_amd import _lib, open_sora_plan_ops, ops, vchitect_ops

        self.lines, self._lib = [], _lib
        real = ops._call

        def spy(name, *args):
            rec = [name]
            for v, kind in zip(args, _lib.SIGNATURES[name][:-1]):
                if isinstance(v, ctypes.Array):
                    rec.append("g" + ",".join(str(int(x)) for x in v))
                elif kind is ctypes.c_void_p or kind is ctypes.c_char_p:
                    rec.append("p" if v is not None else "0")          # an address: only whether there is one
                elif kind is ctypes.c_float:
                    rec.append("f" + struct.pack("<f", float(v)).hex())
                else:
                    rec.append("i" + str(int(v)))
            self.lines.append(" ".join(rec))
            return real(name, *args)

        for m in (ops, vchitect_ops, open_sora_plan_ops):
            m._call = spy

    def digest(self):
        h, n = hashlib.sha256("\n".join(self.lines).encode()).hexdigest(), len(self.lines)
        self.lines = []
        return h, n


def cases(dev):
    """(name, thunk) pairs; every thunk builds its decoder and returns the output tensor."""
    from videosys_amd import vae_cogvideox as VC, vae_open_sora as VO, vae_open_sora_plan as VP, vae_sd3 as V3, vae_svd_temporal as VS

    load = lambda f: torch.load(os.path.join(GOLDEN, f), weights_only=True)
    rnd = lambda seed, *shape: torch.randn(*shape, generator=torch.Generator().manual_seed(seed))
    out = []

    gd = load("opensora_vae_small.pt")
    osv = lambda: VO.OpenSoraVAE(VO.synth_state_dict(gd["seed"]), device=dev, frames_per_launch=8)
    out.append(("open_sora.decode", lambda: osv().decode(gd["z"].to(dev), gd["num_frames"])))
    out.append(("open_sora.decode.frames_15_19", lambda: osv().decode(gd["z"].to(dev), gd["num_frames"], frames=(15, 19))))
    ge = load("opensora_vae_encode_small.pt")

    def encode():
        g = torch.Generator().manual_seed(ge["noise_seed"])
        vae = VO.OpenSoraVAE(VO.synth_state_dict(ge["seed"], encoder=True), device=dev)
        return vae.encode(ge["x"].to(dev), noise_fn=lambda shape: torch.randn(shape, generator=g))

    out.append(("open_sora.encode", encode))

    def latte_2d():
        pre = "spatial_vae.module."
        sd = {k[len(pre):]: v for k, v in VO.synth_state_dict(3).items() if k.startswith(pre)}
        lat = (rnd(8, 1, 4, 3, 4, 6) * 0.18215 * 3).to(torch.bfloat16)
        return VO.AutoencoderKLDecoder(sd, device=dev, frames_per_launch=2).decode(lat.to(dev))

    out.append(("autoencoder_kl.decode", latte_2d))

    def svd():
        lat = (rnd(5, 1, 4, 5, 8, 8) * 0.18215 * 1.5).to(torch.bfloat16)
        return VS.AutoencoderKLTemporalDecoder(VS.synth_state_dict(7), device=dev, decode_chunk_size=3).decode(lat.to(dev))

    out.append(("svd_temporal.decode", svd))
    sd3 = lambda: V3.AutoencoderKLSD3Decoder(V3.synth_state_dict(5), device=dev, frames_per_launch=2)
    z3 = rnd(11, 3, 16, 6, 10)
    out.append(("sd3.decode", lambda: sd3().decode(z3.to(dev))[0].contiguous()))
    out.append(("sd3.decode_u8", lambda: sd3().decode_u8((z3 * 1.5305)[None].to(dev))))
    gc = load("cogvideox_vae_small.pt")

    def cog(tiling):
        vae = VC.CogVideoXVAE(VC.synth_state_dict(gc["seed"]), device=dev, sample_height=gc["sample"][0], sample_width=gc["sample"][1],
                              use_tiling=tiling)
        return vae.decode(gc["z"].to(dev))

    out.append(("cogvideox.decode", lambda: cog(False)))
    out.append(("cogvideox.decode.tiled", lambda: cog(True)))
    gp = load("osp_vae_small.pt")
    sdp = VP.synth_state_dict(gp["seed"], gp["hidden_size"])

    def plan(z, tiling=None):
        w = VP.CausalVAEModelWrapper(sdp, device=dev)
        for k, v in (tiling or {}).items():
            setattr(w.vae, k, v)
        if tiling:
            w.vae.enable_tiling()
        return w.decode(z.to(dev))

    z = gp["z"]
    out.append(("open_sora_plan.a", lambda: plan(z)))
    out.append(("open_sora_plan.b.tiled", lambda: plan(z, gp["tiling"])))
    out.append(("open_sora_plan.c", lambda: plan(z[:, :, :1])))
    out.append(("open_sora_plan.d", lambda: plan(z[:, :, :2])))
    out.append(("open_sora_plan.edge_3x2", lambda: plan(z[:, :, :2, :3, :2].contiguous())))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cpu", action="store_true", help="only the synth_state_dict hashes (no GPU)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {"synth_state_dict": synth_hashes()}
    if not args.cpu:
        assert torch.cuda.is_available(), "the cases need a HIP device (use --cpu for the weight hashes alone)"
        dev = torch.device("cuda:0")
        tr = Trace()
        res["cases"] = {}
        for name, thunk in cases(dev):
            tr.lines = []
            with torch.no_grad():
                y = thunk()
            torch.cuda.synchronize()
            th, n = tr.digest()
            res["cases"][name] = {"output": tensor_hash(y), "trace": th, "launches": n}
            print(f"[vae_host_trace] {name}: {n} launches", file=sys.stderr, flush=True)
    text = json.dumps(res, indent=1, sort_keys=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
