"""GPU: the split-f16 convolution kernels (csrc/convs16.hip, convs16d.hip, convs16u.hip, s16_cvrows.h through convs16.hip / convs16w.hip) pinned
BIT FOR BIT to the build of the commit before their weights moved into AGPRs: sha256 of the launch's whole output -- the RS16
storage with its halo and the slack behind the last unit, the blocked fp32 storage, or the fused head's S buffer -- and the guard word.

PARENT is the commit whose library produced DIGESTS on an MI355X: tools/experiments/exp_agpr.py --record, run with --base-lib = that
commit's build, prints the table below (and compares this tree's build with it, launch by launch).  Inputs and weights are closed-form
(disprcnn_amd.utils.synth.hash_uniform), so the digests do not depend on a random generator's implementation.

Shapes: the smallest at which a form runs all its step kinds -- N = 9 puts two units on one XCD's column worker (a column change inside the
pipeline), D = 4 walks a phantom plane behind the last real one, the head needs D >= 6; the 14- and 7-wide tiles at both channel counts with
and without residual; the stride-2 and transposed kernels in the two instantiations of the headline step; the cost-volume layer in its
one-row and two-row forms."""
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

PARENT = "08509a081d410072d2d0282bb4e5f22f32edd15f"

# id: (kind, N, cin, cout, D, H, W, relu, flag); D, H, W = the INPUT dims; flag: "res" residual, "y32" blocked fp32 output, "head" fused head
CASES = {
    "s1-plain": ("s1", 9, 32, 32, 4, 3, 28, 1, None),
    "s1-res": ("s1", 9, 32, 32, 4, 3, 28, 1, "res"),
    "s1-y32": ("s1", 9, 32, 32, 4, 3, 28, 1, "y32"),
    "s1-head-9": ("s1", 9, 32, 32, 6, 3, 28, 1, "head"),
    "s1-head-wide": ("s1", 1, 32, 32, 6, 2, 56, 1, "head"),
    "s1-32-w14": ("s1", 9, 32, 32, 3, 4, 14, 1, None),
    "s1-32-w14-res": ("s1", 9, 32, 32, 3, 4, 14, 1, "res"),
    "s1-64-w14": ("s1", 9, 64, 64, 3, 4, 14, 1, None),
    "s1-64-w14-res": ("s1", 9, 64, 64, 3, 4, 14, 1, "res"),
    "s1-32-w7": ("s1", 9, 32, 32, 3, 4, 7, 1, None),
    "s1-32-w7-res": ("s1", 9, 32, 32, 3, 4, 7, 1, "res"),
    "s1-64-w7": ("s1", 9, 64, 64, 3, 4, 7, 1, None),
    "s1-64-w7-res": ("s1", 9, 64, 64, 3, 4, 7, 1, "res"),
    "s2-conv1": ("s2", 9, 32, 64, 4, 8, 28, 1, None),          # convs16d_kernel<2,2,14,3,true,true>
    "s2-conv3": ("s2", 9, 64, 64, 4, 4, 14, 1, None),          # convs16d_kernel<4,4,7,2,true,false>
    "up-conv5": ("up", 9, 64, 64, 2, 2, 7, 1, "res"),          # convs16u_kernel<4,7>
    "up-conv6": ("up", 9, 64, 32, 2, 4, 14, 0, "res"),         # convs16u_kernel<2,14>
    "cv-one-row": ("cv1", 2, 64, 32, 3, 4, 28, 1, None),       # convs16_kernel<4,true,...>
    "cv-two-rows": ("cv2", 2, 64, 32, 3, 4, 28, 1, None),      # convs16w_kernel<4,true>
}

# id: (sha256 of the output storage, guard word) -- from PARENT's build
DIGESTS = {
    "s1-plain": ("ca51c09de86a39b502499d9e346b2fee87b35f52a3519b34a5cd73a8b6d4a775", 0),
    "s1-res": ("bcc2fbf463342613ea794afb31cec27b544832c20c415421310612ce3ba4efa3", 0),
    "s1-y32": ("73433d865d9e8b24778e79aefd598c633778a9544f34709671d1bd272b04faee", 0),
    "s1-head-9": ("244f952c8a3d56c39caf501baa22f05288f31a88098554de43657bd55e8d9e41", 0),
    "s1-head-wide": ("f7a433224e82c8e7eff7b30eec9d1721ea49f21ac66eca29c07e3ed11f915d2d", 0),
    "s1-32-w14": ("3e14914f4c344896692a374e0ae91bf41b05cab5f3443bc9ba91fc70c373ba00", 0),
    "s1-32-w14-res": ("6f09c8b40483f6e9b3ba79d06844df9fdfe06a0bfcad86e366951d4d6058955e", 0),
    "s1-64-w14": ("6f63b254c56700d7063598ff7fdbef869ae7cd158d7373264bf5fdab55bd1ffc", 0),
    "s1-64-w14-res": ("663d5004726150f8efd1b9af7ff7c25bfda20f8fc1845238a40c0aa546e40f23", 0),
    "s1-32-w7": ("5603fa03841ee164243cde11bed0b2a72a5e9ef494ccab5ade329a25edd9e8bb", 0),
    "s1-32-w7-res": ("1590514e03fe17d29c658959e0f4318420876d855757cca571f83ab89ff36f93", 0),
    "s1-64-w7": ("171130bb9486e81c3c1fb4bf0d23b0136d4d528832a4711b5572e0f35839b580", 0),
    "s1-64-w7-res": ("33ce46253ff828b6b8e09a2c2435a13ab713d498027346bcb0a776018c79431c", 0),
    "s2-conv1": ("529c208858cf7398c0c80754e44c47fe0b4c88a8e630752e6d67dadb6c19252e", 0),
    "s2-conv3": ("06e2a733dbbe046898ccd128c3f553fb8fed6ce9cbb2c8c918d2b825dbbb9d3e", 0),
    "up-conv5": ("eda9684de8f44d31d16769b95e75861ef6ea3c9123cc61b3ffec39b8a078bfb6", 0),
    "up-conv6": ("cda00a862d1caf1c41e4c2683bf63209ae63a85ec59f4e5f31e8ee42617edd6e", 0),
    "cv-one-row": ("3b812e184f33e7aa8316b9b7aaccc12c9cc1a7068b996a05a16d778d9c47d881", 0),
    "cv-two-rows": ("2a8528d88890ee9820f079a261bca2409731e67a1627d0f95f9a8368cfda267d", 0),
}

FUNCS = {"s1": "drc_conv3d_k3_s16_fwd", "cv1": "drc_conv3d_k3_s16_fwd", "cv2": "drc_conv3d_k3_s16_wide_fwd", "s2": "drc_conv3d_k3s2_s16_fwd",
         "up": "drc_deconv3d_k3s2_s16_fwd"}


def load(path):
    """Another build of the library, with the signatures of the entry points used here."""
    h = C.CDLL(path)
    for name in set(FUNCS.values()):
        fn = getattr(h, name)
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p]
    return h


class Launch:
    """Inputs, weights and a fresh output of one case; run(lib) launches it and returns (output storage, guard word)."""

    def __init__(self, dev, cid, spec=None, rand=False):
        """spec: a tuple like those of CASES (default: CASES[cid]); rand: uniform values from torch's generator on the device instead of the
        closed-form ones (large timing shapes of tools/experiments/exp_agpr.py: the closed form is computed on the host)."""
        kind, N, cin, cout, D, H, W, relu, flag = spec or CASES[cid]
        self.kind, self.N, self.cin, self.cout, self.D, self.H, self.W, self.relu, self.flag, self.dev = kind, N, cin, cout, D, H, W, relu, flag, dev
        if rand:
            g = torch.Generator(device=dev).manual_seed(7)
            u = lambda name, shape, lo=-1.0, hi=1.0: torch.rand(shape, generator=g, device=dev) * (hi - lo) + lo
        else:
            u = lambda name, shape, lo=-1.0, hi=1.0: hash_uniform(f"pins:{cid}:{name}", shape, lo, hi).to(dev)
        if kind == "up":
            w = u("w", (cin, cout, 3, 3, 3)) * (6.0 / (27 * cin / 8)) ** 0.5
            self.od = (2 * D, 2 * H, 2 * W)
            self.wp, wexp = s16.pack_weight_s16(w.transpose(0, 1).contiguous())
        else:
            w = u("w", (cout, cin, 3, 3, 3)) * (6.0 / (27 * cin)) ** 0.5
            self.od = (D // 2, H // 2, W // 2) if kind == "s2" else (D, H, W)
            self.wp, wexp = s16.pack_weight_s16(w)
        self.sc = (u("scale", (cout,), 0.5, 1.5) * (2.0 ** -wexp)).contiguous()
        self.sh = u("shift", (cout,), -0.1, 0.1)
        self.x16 = self.l16 = self.r16 = self.res = self.hp = None
        if kind in ("cv1", "cv2"):
            self.l16 = E.RS16(N, 32, 1, H, W, 0, dev).from_dense(u("left", (N, 32, H, W)))
            self.r16 = E.RS16(N, 32, 1, H, W, 0, dev).from_dense(u("right", (N, 32, H, W)))
        else:
            self.x16 = E.RS16(N, cin, D, H, W, 1, dev).from_dense(u("x", (N, cin, D, H, W)))
        if flag == "res":
            self.res = E.RS16(N, cout, *self.od, 1, dev).from_dense(u("res", (N, cout) + self.od))
        if flag == "head":
            hp, _ = s16.pack_head_weight_s16(u("w1", (1, 32, 3, 3, 3)) * (6.0 / 27) ** 0.5)
            self.hp = hp.to(dev)

    def out(self):
        if self.flag == "head":
            return torch.zeros(self.N, self.D, self.H, self.W, 12, device=self.dev)
        if self.flag == "y32":
            return E.Blocked(self.N, self.cout, *self.od, 1, 1, 1, self.dev).storage
        return E.RS16(self.N, self.cout, *self.od, 1, self.dev).storage

    def launch(self, lib, y, word=None, lo4=0):
        P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        S = lambda t: P(t.storage) if t is not None else None
        head, y32 = self.flag == "head", self.flag == "y32"
        prm = DrcS16ConvParams(S(self.x16), P(self.wp), P(self.sc), P(self.sh), S(self.res), None if head or y32 else P(y), P(y) if y32 else None,
                               S(self.l16), S(self.r16), self.N, self.D, self.H, self.W, self.cin, self.cout, self.relu, lo4,
                               0x800 if self.kind == "cv1" else 1,      # (the library's experiment bit: keep the one-row kernel)
                               P(y) if head else None, P(self.hp), P(word))
        _lib.check(getattr(lib, FUNCS[self.kind])(C.byref(prm), C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)), FUNCS[self.kind])

    def run(self, lib):
        y, word = self.out(), torch.zeros(1, dtype=torch.int32, device=self.dev)
        self.launch(lib, y, word)
        torch.cuda.synchronize()
        return y, word


def digest(y, word):
    return hashlib.sha256(y.cpu().numpy().tobytes()).hexdigest(), int(word.item())


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def test_every_case_has_a_recorded_digest():
    assert sorted(DIGESTS) == sorted(CASES)


@pytest.mark.parametrize("cid", list(CASES))
def test_output_and_guard_word_equal_the_parent_builds(dev, cid):
    y, word = Launch(dev, cid).run(_lib.lib())
    assert y.abs().max().item() > 0.1 and torch.isfinite(y).all()          # (a launch that wrote nothing would be "equal" only to itself)
    assert digest(y, word) == DIGESTS[cid], f"{cid}: differs from the build of {PARENT[:7]}"
