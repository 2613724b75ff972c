"""GPU: the cost-volume layer (csrc/s16_cvrows.h through convs16.hip / convs16w.hip) pinned BIT FOR BIT to the build of the commit before its
assembly loop changed (left taps in registers, a masked term as fma(A, 0, +0), right-column offsets carried from plane to plane):
sha256 of the launch's whole RS16
output storage, halo included, and the guard word, through the three entry forms -- drc_conv3d_k3_s16_fwd, the same with dil = 0x800 (the
one-row kernel kept), drc_conv3d_k3_s16_wide_fwd.

PARENT is the commit whose library produced DIGESTS on an MI355X: tools/experiments/exp_cvrows_asm.py --record, run with --base-lib = that
commit's build, prints the table below (after checking that the parent's three entry forms agree with each other) and compares this tree's
build with it in the same process.  Inputs and weights are closed-form (disprcnn_amd.utils.synth.hash_uniform).

Shapes: those of tests/test_hip_s16_cvrows.py and (2, 5, 6, 28, 3): odd D, so the two plane parities of a row store different numbers of
planes, and several rows per workgroup.  Between them: every read alignment (12 planes x lo4), two right-map tiles, masked x tiles, D = 1
and 2 (a parity that stores nothing), more than 32 planes, consecutive tasks of a workgroup that change x tile and unit (the A registers
reload, the carried offsets restart)."""
import ctypes as C
import hashlib

import pytest
import torch

from disprcnn_amd import _lib
from disprcnn_amd import engine as E
from disprcnn_amd import s16
from disprcnn_amd._lib import DrcS16ConvParams
from disprcnn_amd.utils.synth import hash_uniform

pytestmark = pytest.mark.gpu

PARENT = "ef35528b7e20011a5fbb46b5a4b0a9cc25a26f92"

# id: (N, D, H, W, lo4)
SHAPES = {
    "configA": (3, 12, 28, 28, 0),
    "configB": (1, 24, 56, 56, -12),
    "lo4-6": (2, 12, 28, 28, -6),
    "lo4+9-oddH": (2, 6, 5, 28, 9),
    "masked-planes": (2, 6, 5, 16, -18),
    "masked-x-tile": (2, 8, 12, 40, 2),
    "three-x-tiles": (3, 4, 7, 64, -1),
    "D1": (2, 1, 3, 16, 0),
    "D2": (2, 2, 4, 40, -1),
    "D3-N9": (9, 3, 9, 28, 1),
    "D40": (1, 40, 4, 28, -20),
    "oddD-rows": (2, 5, 6, 28, 3),
}

# entry form: (C entry point, dil)
ENTRIES = {"dispatch": ("drc_conv3d_k3_s16_fwd", 1), "one-row": ("drc_conv3d_k3_s16_fwd", 0x800), "wide": ("drc_conv3d_k3_s16_wide_fwd", 1)}

# id: (sha256 of the output storage, guard word) -- from PARENT's build, the same through its three entry forms
DIGESTS = {
    "configA": ("7944279e166220d09b04eb91c3be952f9e60e23411ed261fb8d75f2075b72251", 0),
    "configB": ("d1b9829053a2c772c9b663df7a3e07101ec22f116267f3d9a14fdbbfbeff069e", 0),
    "lo4-6": ("3b01b2038513649e17675ac7bc9f3bf29c0724eeb6db4c3ebb16280439f389c6", 0),
    "lo4+9-oddH": ("eb0205309ac60fc96e9988b3b3c6160d70b5d8d69a420e87b14395e93f737346", 0),
    "masked-planes": ("56fa03904953627f2cc3314097d52c193c198176d7a44dc7b66fc26e23dd134e", 0),
    "masked-x-tile": ("323650f4b9112a9244c288d3e741be9a94ee93e22e558025acf2dcfd655177bf", 0),
    "three-x-tiles": ("842e450d61c3c053f3beb6f03834015fae20fc602cfb43271020ae06883789a7", 0),
    "D1": ("24ccd924c59de4541361fa88c834daea396651dd0ca6ff7f122500db3a0b6890", 0),
    "D2": ("015af23cebbbe448e00f4cae8fec487702dfcc71451eb25f5851743f96a70c96", 0),
    "D3-N9": ("fcb6c7667db10b634f6cd5b11640f3747a059b7183534efd6d6535ffc2028888", 0),
    "D40": ("9b69a2a16ac2226879c52df143e2e172b9c94faaf3504103d99884769483688a", 0),
    "oddD-rows": ("f59674915699945f375a30e49a28afc998468394aaa3a73249dfb6dc3e271055", 0),
}


def load(path):
    """Another build of the library, with the signatures of the entry points used here."""
    h = C.CDLL(path)
    for name, _ in ENTRIES.values():
        fn = getattr(h, name)
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p]
    return h


class Layer:
    """Inputs and weights of one shape; run(lib, entry) launches it into a fresh output and returns (output storage, guard word)."""

    def __init__(self, dev, sid, shape=None):
        N, D, H, W, lo4 = shape or SHAPES[sid]
        self.dev, self.N, self.D, self.H, self.W, self.lo4 = dev, N, D, H, W, lo4
        u = lambda name, shp, lo=-1.0, hi=1.0: hash_uniform(f"cvpins:{sid}:{name}", shp, lo, hi).to(dev)
        self.wp, wexp = s16.pack_weight_s16(u("w", (32, 64, 3, 3, 3)) * (6.0 / (27 * 64)) ** 0.5)
        self.sc = (u("scale", (32,), 0.5, 1.5) * (2.0 ** -wexp)).contiguous()
        self.sh = u("shift", (32,), -0.1, 0.1)
        self.l16 = E.RS16(N, 32, 1, H, W, 0, dev).from_dense(u("left", (N, 32, H, W)))
        self.r16 = E.RS16(N, 32, 1, H, W, 0, dev).from_dense(u("right", (N, 32, H, W)))

    def out(self):
        return E.RS16(self.N, 32, self.D, self.H, self.W, 1, self.dev).storage

    def launch(self, lib, entry, y, word=None):
        name, dil = ENTRIES[entry]
        P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        prm = DrcS16ConvParams(None, P(self.wp), P(self.sc), P(self.sh), None, P(y), None, P(self.l16.storage), P(self.r16.storage),
                               self.N, self.D, self.H, self.W, 64, 32, 1, self.lo4, dil, None, None, P(word))
        _lib.check(getattr(lib, name)(C.byref(prm), C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)), name)

    def run(self, lib, entry):
        y, word = self.out(), torch.zeros(1, dtype=torch.int32, device=self.dev)
        self.launch(lib, entry, y, word)
        torch.cuda.synchronize()
        return y, word


def digest(y, word):
    return hashlib.sha256(y.cpu().numpy().tobytes()).hexdigest(), int(word.item())


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def layers(dev):
    cache = {}

    def get(sid):
        if sid not in cache:
            cache[sid] = Layer(dev, sid)
        return cache[sid]
    return get


def test_every_shape_has_a_recorded_digest():
    assert sorted(DIGESTS) == sorted(SHAPES)


@pytest.mark.parametrize("entry", list(ENTRIES))
@pytest.mark.parametrize("sid", list(SHAPES))
def test_output_and_guard_word_equal_the_parent_builds(dev, layers, sid, entry):
    y, word = layers(sid).run(_lib.lib(), entry)
    assert y.abs().max().item() > 0.01 and torch.isfinite(y).all()         # (a launch that wrote nothing would be "equal" only to itself)
    assert digest(y, word) == DIGESTS[sid], f"{sid} / {entry}: differs from the build of {PARENT[:7]}"
