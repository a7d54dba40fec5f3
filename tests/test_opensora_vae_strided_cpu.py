"""CPU: vsys_conv_causal_tdown2_bf16, the time-stride-2 causal convolution of the Open-Sora v1.2 VAE encoder — in the header with the
reference lines it replaces, exported, in the generated binding, without an op code — and its refusals, each on pointers that are never
dereferenced (every call below returns before any launch)."""
import ctypes
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "vsys_conv_causal_tdown2_bf16"


def test_entry_point_in_header_and_binding_without_an_op_code():
    from videosys_amd import _lib
    from videosys_amd._opcodes import ENTRY_POINTS, OPCODES

    header = open(os.path.join(ROOT, "include", "videosys_amd.h")).read()
    assert f"int {NAME}(void* stream, const void* x," in header and "autoencoder_kl_open_sora.py:107-125,229-236" in header
    assert ENTRY_POINTS[NAME] == ("pplplplpplll", "i") and NAME in _lib.SIGNATURES and NAME not in OPCODES
    assert hasattr(_lib.load(), NAME)


def test_refusals_before_any_launch():
    from videosys_amd import _lib

    lib, P = _lib.load(), 0x10000       # an aligned address that is never dereferenced
    G = lambda *v: (ctypes.c_int64 * 6)(*v)

    def call(x=P, ldx=128, n=1, w=P, ldw=27 * 128, cin=128, cout=128, g=G(4, 8, 8, 0, 0, 256), ldo=128, out=P):
        return getattr(lib, NAME)(None, x, ldx, g, n, w, ldw, None, out, ldo, cin, cout)

    assert call(cout=64, ldo=64) == -1 and call(cin=48, ldw=27 * 48) == -1 and call(ldx=64) == -1 and call(ldw=128) == -1 and call(n=70000) == -1
    assert call(g=G(1, 8, 8, 0, 0, 64)) == -1 and call(g=G(4, 1, 8, 0, 0, 32)) == -1 and call(g=G(4, 8, 1, 0, 0, 32)) == -1
    assert call(g=G(4, 8, 8, 0, 0, 100)) == -1                                                # sample_rows below the grid's frames
    assert call(ldx=1 << 22, g=G(2, 64, 64, 0, 0, 8192)) == -1                                # a tile's source span reaches 2 GiB
    assert call(x=P + 2) == -2 and call(w=P + 8) == -2 and call(out=P + 4) == -2 and call(ldx=132) == -2 and call(ldo=132) == -2
    assert call(x=None) == -3 and call(w=None) == -3 and call(g=None) == -3
    assert call(n=0) == 0 and call(n=0, cin=32, ldw=27 * 32, cout=256, ldo=256, g=G(5, 5, 7, 1, 2, 7 * 63)) == 0   # accepted: nothing to launch
