"""CPU: the render loss (the adjoint in csrc/sphere_render.hip, ``evaluate.render_spheres`` as a differentiable function,
``evaluate.RenderLoss``, ``--lambda_render``) WITHOUT a GPU.

* ``tests/render_grad_oracle.py`` is the adjoint of ``tests/sphere_render_oracle.py``'s render: ``<render(x), g> == <x, vjp(g)>``.
* The three entry points are declared in ``include/emlight_hip_ext.h``, bound in ``_lib.EXT_SIGNATURES`` and exported; the
  first header and its 131 names are untouched.
* The launchers' own argument validation runs against the built library (it returns before anything touches a device).
* The Python layers reach the entry points with arguments that convert to the bound signatures: the HIP library is replaced
  by a recorder (the pattern of ``test_pano_warp_abi.py``, restated here)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import render_grad_oracle as grad_oracle
from tests import sphere_render_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"eml_sphere_render_bwd_work_floats": 4, "eml_sphere_render_bwd_f32": 14, "eml_sphere_mirror_taps_f32": 7}
FORWARD = ["eml_sphere_render_work_floats", "eml_sphere_render_f32"]
BACKWARD = ["eml_sphere_render_bwd_work_floats", "eml_sphere_render_bwd_f32"]
BACKWARD_FIRST_MIRROR = ["eml_sphere_render_bwd_work_floats", "eml_sphere_mirror_taps_f32", "eml_sphere_render_bwd_f32"]


# ------------------------------------------------------------------------------------------------ the oracle is an adjoint
@pytest.mark.parametrize("az", [180.0, 77.3])
def test_oracle_vjp_is_the_adjoint_of_the_oracle_render(az):
    H, W, S, B = 16, 32, 9, 2
    rng = np.random.default_rng([7, int(az)])
    x = rng.standard_normal((B, 3, H, W))
    g = rng.standard_normal((B, 3, 3, S, S))
    assert np.abs(g[..., ~oracle.mask(S)]).min() > 0                  # non-zero outside the disc: must be ignored
    lhs = float(np.sum(oracle.render(x, S, oracle.MATERIALS, az, 50.0) * g))
    rhs = float(np.sum(x * grad_oracle.vjp(g, H, W, S, oracle.MATERIALS, az, 50.0)))
    scale = float(np.sum(np.abs(x) * grad_oracle.abs_vjp(g, H, W, S, oracle.MATERIALS, az, 50.0)))
    print("az %g: <render(x), g> %.17g  <x, vjp(g)> %.17g  scale %.3e" % (az, lhs, rhs, scale))
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs))
    assert abs(lhs) > 1e-3 * scale                                    # not a cancelled zero: the relative bound means something
    # the caller's order and a subset go through the same code
    sub = ("mirror", "diffuse")
    lhs = float(np.sum(oracle.render(x, S, sub, az, 50.0) * g[:, :2]))
    rhs = float(np.sum(x * grad_oracle.vjp(g[:, :2], H, W, S, sub, az, 50.0)))
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs))


def test_oracle_taps_are_the_mirror_of_the_render_oracle():
    """Four exact products of the f32-rounded fractions against the oracle's nested blend: the same numbers in float64; in
    float32 arithmetic (the device's table) each within 3 roundings.  The centre pixel at azimuth 180 wraps its columns, a
    pixel at the lower rim clamps its rows."""
    H, W, S = 16, 32, 9
    idx, w = grad_oracle.taps(H, W, S)
    P = int(oracle.mask(S).sum())
    assert idx.shape == w.shape == (P, 4) and idx.min() >= 0 and idx.max() < H * W
    assert np.abs(w.sum(1) - 1).max() <= 1e-15 and w.min() >= 0
    x = np.random.default_rng(5).random((1, 3, H, W))
    got = np.einsum("pk,cpk->cp", w, x.reshape(3, H * W)[:, idx])
    assert np.abs(got - oracle.mirror(x, S)[0]).max() <= 1e-14
    idx32, w32 = grad_oracle.taps(H, W, S, f32=True)
    assert np.array_equal(idx32, idx) and np.abs(w32 - w).max() <= 3 * 2.0 ** -24
    centre = int(np.flatnonzero(np.flatnonzero(oracle.mask(S).ravel()) == (S // 2) * S + S // 2)[0])
    assert idx[centre, 0] % W == W - 1 and idx[centre, 1] % W == 0
    assert not np.any(idx[:, 0] == idx[:, 2])                         # no reflection within half a texel of the pole here
    idx, w = grad_oracle.taps(12, 24, 33)
    clamped = idx[:, 0] == idx[:, 2]
    assert clamped.sum() == 4 and np.all(idx[clamped, 0] // 24 == 11) and np.all(idx[clamped, 1] == idx[clamped, 3])
    assert grad_oracle.max_taps_on_a_texel(12, 24, 33) == 25


# ------------------------------------------------------------------------------------------------ where the symbols live
@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as g
    g.build()
    from emlight_amd import _lib
    return _lib.lib()


def test_symbols_are_declared_in_the_extension_header_bound_and_exported(built_lib):
    from emlight_amd import _lib
    ext = open(os.path.join(ROOT, "include", "emlight_hip_ext.h")).read()
    first = open(os.path.join(ROOT, "include", "emlight_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", ext, flags=re.S)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in NEW.items():
        decl = re.search(r"\b%s\((.*?)\);" % name, code, re.S).group(1)
        assert len(decl.split(",")) == len(_lib.EXT_SIGNATURES[name][1]) == nargs, name
        assert hasattr(handle, name), "libemlight_hip.so does not export %s" % name
        assert getattr(built_lib, name).argtypes == _lib.EXT_SIGNATURES[name][1]
        assert name not in first and name not in _lib.SIGNATURES
    assert _lib.EXT_SIGNATURES["eml_sphere_render_bwd_work_floats"][0] is ctypes.c_size_t
    # each declaration cites the definition, as eml_sphere_render_f32 does
    comments = re.findall(r"/\*.*?\*/", ext, flags=re.S)
    assert sum("DESIGN.md section 15" in c for c in comments) >= 2
    # the first header, its table and the ABI version are untouched
    assert len(_lib.SIGNATURES) == 131 and not set(_lib.SIGNATURES) & set(_lib.EXT_SIGNATURES)
    assert int(re.search(r"#define EML_ABI_VERSION (\d+)", first).group(1)) == _lib.ABI_VERSION == 31
    assert len(set(re.findall(r"\b(eml_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", first, flags=re.S)))) == 131
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "RenderLoss" in readme and "--lambda_render" in readme and all(n in readme for n in NEW)


def test_launcher_argument_validation_without_gpu(built_lib):
    L = built_lib
    one = ctypes.c_void_p(16)

    def bwd(g=one, B=1, H=16, W=32, S=8, az=180.0, mask=3, m=50.0, cp=None, cs=None, cw=None, dpano=one, work=one):
        return L.eml_sphere_render_bwd_f32(g, B, H, W, S, az, mask, m, cp, cs, cw, dpano, work, None)

    for kw in ({"g": None}, {"dpano": None}, {"work": None}):
        assert bwd(**kw) == -1 and b"null" in L.eml_last_error(), kw
    assert bwd(W=33) == -1 and b"W == 2H" in L.eml_last_error()
    assert bwd(H=0, W=0) == -1 and b"W == 2H" in L.eml_last_error()
    assert bwd(S=1) == -1 and b"S must be" in L.eml_last_error()
    for mask in (0, 8, -1):
        assert bwd(mask=mask) == -1 and b"materials mask" in L.eml_last_error(), mask
    for mask in (4, 5, 7):                                                   # a mirror bit without its table
        for kw in ({}, {"cp": one, "cs": one}, {"cs": one, "cw": one}, {"cp": one, "cw": one}):
            assert bwd(mask=mask, **kw) == -1 and b"mirror_csr" in L.eml_last_error(), (mask, kw)
    assert bwd(m=-0.5) == -1 and b"phong" in L.eml_last_error()
    assert bwd(m=float("nan")) == -1 and b"phong" in L.eml_last_error()
    for kw in ({"B": -1}, {"B": 4097}, {"S": 1025}, {"H": 4097, "W": 8194}):  # the forward's limits
        assert bwd(**kw) == -1 and b"grid limits" in L.eml_last_error(), kw
    assert bwd(work=ctypes.c_void_p(20)) == -1 and b"aligned" in L.eml_last_error()
    assert bwd(B=0) == 0 and bwd(B=0, mask=7, cp=one, cs=one, cw=one) == 0    # empty batch: nothing to launch
    # texel table (4 H W) + pixel records (8 P): the summation is not split, so nothing depends on the batch
    P8, P33 = int(oracle.mask(8).sum()), int(oracle.mask(33).sum())
    work = L.eml_sphere_render_bwd_work_floats
    assert work(0, 16, 32, 8) == 0 and work(1, 16, 33, 8) == 0 and work(1, 16, 32, 1) == 0
    assert work(3, 16, 32, 8) == 4 * 512 + 8 * P8 and work(2, 12, 24, 33) == 4 * 288 + 8 * P33
    assert work(1, 128, 256, 16) == work(5, 128, 256, 16)

    def taps(H=16, W=32, S=8, az=180.0, idx=one, wgt=one):
        return L.eml_sphere_mirror_taps_f32(H, W, S, az, idx, wgt, None)

    for kw in ({"idx": None}, {"wgt": None}):
        assert taps(**kw) == -1 and b"null" in L.eml_last_error(), kw
    assert taps(W=31) == -1 and b"W == 2H" in L.eml_last_error()
    for kw in ({"S": 1}, {"S": 1025}, {"H": 4097, "W": 8194}, {"az": float("nan")}):
        assert taps(**kw) == -1 and b"grid limits" in L.eml_last_error(), kw


# ------------------------------------------------------------------------------------------------ recorder
class _Recorder:
    def __init__(self, signatures):
        self.signatures, self.calls, self.args = signatures, [], []

    def __getattr__(self, name):
        if name not in self.signatures:
            raise AttributeError(name)
        restype, argtypes = self.signatures[name]

        def call(*args):
            assert len(args) == len(argtypes), "%s takes %d arguments, call site passes %d" % (name, len(argtypes), len(args))
            for k, (a, t) in enumerate(zip(args, argtypes)):
                try:
                    t.from_param(a)
                except (TypeError, ctypes.ArgumentError) as e:
                    raise AssertionError("%s: argument %d (%r) does not convert to %s" % (name, k, a, t.__name__)) from e
            self.calls.append(name)
            self.args.append((name, args))
            return 64 if restype is ctypes.c_size_t else 0
        return call

    def of(self, name):
        return [a for n, a in self.args if n == name]


@pytest.fixture
def recorder(monkeypatch):
    from emlight_amd import _lib, evaluate

    def require(t, name, dtype=None):      # the dtype check stays, the device check goes
        if t.dtype != (dtype or torch.float32):
            raise _lib.EmlightHipError("%s must be %s" % (name, dtype or torch.float32))
        return t.contiguous()
    rec = _Recorder({**_lib.SIGNATURES, **_lib.EXT_SIGNATURES})
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    monkeypatch.setattr(_lib, "current_stream", lambda: None)
    monkeypatch.setattr(_lib, "require_gpu_tensor", require)
    monkeypatch.setattr(evaluate, "_MIRROR_CSR", {})       # every test meets its geometries for the first time
    return rec


# eml_sphere_render_bwd_f32(grad_out, B, H, W, S, view_azimuth_deg, materials_mask, phong_m, csr_ptr, csr_src, csr_w, dpano,
#                           work, stream)
def test_render_spheres_without_grad_makes_todays_calls(recorder):
    from emlight_amd.evaluate import lighting_metrics, render_spheres
    out = render_spheres(torch.rand(3, 3, 16, 32), size=9)
    assert out.shape == (3, 3, 3, 9, 9) and not out.requires_grad and recorder.calls == FORWARD
    recorder.calls.clear()
    x = torch.rand(2, 3, 16, 32, requires_grad=True)
    with torch.no_grad():
        assert not render_spheres(x, size=9).requires_grad
    assert recorder.calls == FORWARD
    recorder.calls.clear()
    m = lighting_metrics(x, torch.rand(2, 3, 16, 32), size=8)              # scores: rendered under no_grad
    assert recorder.calls == FORWARD + ["eml_sphere_render_metrics_f64"] and not any(v.requires_grad for v in m.values())


def test_render_spheres_with_grad_adds_the_backward_call(recorder):
    from emlight_amd.evaluate import render_spheres
    x = torch.rand(3, 3, 16, 32, requires_grad=True)
    out = render_spheres(x, size=9, view_azimuth_deg=77, phong_exponent=3)
    assert out.shape == (3, 3, 3, 9, 9) and out.requires_grad and recorder.calls == FORWARD
    assert recorder.of("eml_sphere_render_f32")[0][1:8] == (3, 16, 32, 9, 77.0, 7, 3.0)
    g = torch.rand(3, 3, 3, 9, 9)
    out.backward(g)
    assert recorder.calls == FORWARD + BACKWARD_FIRST_MIRROR
    assert recorder.of("eml_sphere_render_bwd_work_floats")[0] == (3, 16, 32, 9)
    assert recorder.of("eml_sphere_mirror_taps_f32")[0][:4] == (16, 32, 9, 77.0)
    a = recorder.of("eml_sphere_render_bwd_f32")[0]
    assert a[1:8] == (3, 16, 32, 9, 77.0, 7, 3.0) and isinstance(a[5], float) and isinstance(a[7], float)
    assert all(p is not None for p in a[8:13]) and a[13] is None
    assert x.grad.shape == (3, 3, 16, 32) and x.grad.dtype == torch.float32 and x.grad.data_ptr() == a[11].value   # 3B columns
    # the same geometry again: the tap table is kept
    recorder.calls.clear()
    render_spheres(x, size=9, view_azimuth_deg=77, phong_exponent=3).sum().backward()
    assert recorder.calls == FORWARD + BACKWARD
    # no mirror: no table; the caller's order goes through the stack of slices, the kernel sees its own order
    for names, bits in ((("diffuse",), 1), (("glossy", "diffuse"), 3), (("mirror", "diffuse"), 5), ("mirror", 4)):
        recorder.calls.clear(), recorder.args.clear()
        y = torch.rand(1, 3, 4, 8, requires_grad=True)
        out = render_spheres(y, size=4, materials=names)
        assert out.shape == (1, 1 if isinstance(names, str) else len(names), 3, 4, 4)
        out.sum().backward()
        b = recorder.of("eml_sphere_render_bwd_f32")[0]
        assert b[1:5] == (1, 4, 8, 4) and b[6] == bits == recorder.of("eml_sphere_render_f32")[0][6]
        assert (b[8] is None and b[9] is None and b[10] is None) == (not bits & 4)
        assert ("eml_sphere_mirror_taps_f32" in recorder.calls) == (bits == 5)     # 4 meets 5's geometry again
        assert y.grad.shape == (1, 3, 4, 8)
    # an empty batch launches nothing, forward or backward
    recorder.calls.clear()
    z = torch.rand(0, 3, 4, 8, requires_grad=True)
    render_spheres(z, size=4).sum().backward()
    assert recorder.calls == [] and z.grad.shape == (0, 3, 4, 8)


def test_render_loss_renders_2b_forward_and_b_backward(recorder):
    from emlight_amd.evaluate import RenderLoss
    crit = RenderLoss(size=8)
    assert isinstance(crit, torch.nn.Module) and not list(crit.parameters()) and not list(crit.buffers())
    assert (crit.size, crit.materials, crit.view_azimuth_deg, crit.phong_exponent) == (8, ("diffuse", "glossy"), 180.0, 50.0)
    assert RenderLoss().size == 32
    pred = torch.rand(3, 3, 16, 32, requires_grad=True)
    true = torch.rand(3, 3, 16, 32, requires_grad=True)
    loss = crit(pred, true)
    assert loss.shape == () and loss.requires_grad and recorder.calls == FORWARD
    assert recorder.of("eml_sphere_render_work_floats")[0] == (6, 16, 32, 8)
    assert recorder.of("eml_sphere_render_f32")[0][1:8] == (6, 16, 32, 8, 180.0, 3, 50.0)        # one call of 2B images
    loss.backward()
    assert recorder.calls == FORWARD + BACKWARD
    assert recorder.of("eml_sphere_render_bwd_f32")[0][1:8] == (3, 16, 32, 8, 180.0, 3, 50.0)   # the prediction's 3B columns
    assert pred.grad.shape == (3, 3, 16, 32) and true.grad is None
    # a prediction that asks for no gradient: the forward's calls alone
    recorder.calls.clear()
    assert not crit(pred.detach(), true).requires_grad and recorder.calls == FORWARD
    # all three materials in any order: the kernel's mask, the tap table once
    recorder.calls.clear()
    RenderLoss(size=4, materials=("mirror", "glossy", "diffuse"), view_azimuth_deg=10, phong_exponent=2)(pred, true).backward()
    assert recorder.calls == FORWARD + BACKWARD_FIRST_MIRROR
    assert recorder.of("eml_sphere_render_bwd_f32")[-1][1:8] == (3, 16, 32, 4, 10.0, 7, 2.0)
    for bad in ((pred, true[:2]), (pred[:0], true[:0]), (torch.rand(1, 3, 4, 9), torch.rand(1, 3, 4, 9))):
        with pytest.raises(ValueError):
            crit(*bad)
    for kw in ({"size": 1}, {"materials": ()}, {"materials": ("chrome",)}, {"phong_exponent": -1.0}):
        with pytest.raises(ValueError):
            RenderLoss(**kw)


def test_cpu_tensors_are_refused():
    from emlight_amd import _lib
    from emlight_amd.evaluate import RenderLoss
    with pytest.raises(_lib.EmlightHipError):
        RenderLoss(size=4)(torch.rand(1, 3, 4, 8, requires_grad=True), torch.rand(1, 3, 4, 8))


# ------------------------------------------------------------------------------------------------ the generator's loss dict
class _StubModel:
    """``Pix2PixModel.compute_generator_loss`` on stand-ins for the networks: what it calls and which keys it returns."""

    def __init__(self, opt, fake):
        from emlight_amd.GenProjector.pix2pix_model import Pix2PixModel
        self.opt, self.fake = opt, fake
        self._render_loss = lambda: Pix2PixModel._render_loss(self)
        self.loss = lambda *a: Pix2PixModel.compute_generator_loss(self, *a)

    def generate_fake(self, inp, crop):
        return self.fake

    def discriminate_raw(self, inp, fake, real, for_generator=False):
        return [[torch.cat([fake, real], 0).mean((1, 2, 3))]]                # one discriminator, no intermediate maps

    def criterionGAN(self, pred, target_is_real, for_discriminator=True):
        return -pred[0][0].mean()


def test_generator_loss_has_a_render_term_only_when_asked(recorder):
    from emlight_amd.GenProjector.networks import default_options
    fake = torch.rand(2, 3, 16, 32, requires_grad=True)
    inp, crop, real, mask = torch.rand(2, 3, 16, 32), torch.rand(2, 3, 16, 16), torch.rand(2, 3, 16, 32), torch.rand(2, 1, 16, 32)
    opt = default_options()
    assert (opt.lambda_render, opt.render_size) == (0.0, 32)
    absent = default_options()
    del absent.lambda_render, absent.render_size
    for o in (opt, absent):
        losses, out = _StubModel(o, fake).loss(inp, crop, real, mask)
        assert list(losses) == ["GAN", "GAN_Feat", "COS"] and out is fake
        assert not [c for c in recorder.calls if "sphere_render" in c or "mirror_taps" in c]
    model = _StubModel(default_options(lambda_render=0.5, render_size=8), fake)
    losses, _ = model.loss(inp, crop, real, mask)
    assert list(losses) == ["GAN", "GAN_Feat", "COS", "Render"] and losses["Render"].shape == ()
    assert recorder.calls == FORWARD and recorder.of("eml_sphere_render_f32")[0][1:8] == (4, 16, 32, 8, 180.0, 3, 50.0)
    sum(losses.values()).mean().backward()
    assert recorder.calls == FORWARD + BACKWARD and recorder.of("eml_sphere_render_bwd_f32")[0][1:5] == (2, 16, 32, 8)
    assert model._render_loss() is model._render_loss()                      # one criterion per model


# ------------------------------------------------------------------------------------------------ command lines
def test_render_flags_parse_on_the_projector_and_the_joint_parsers(capsys):
    from emlight_amd import joint
    from emlight_amd.GenProjector import networks, options
    for parser in (options.train_parser(), joint.build_parser()):
        args = parser.parse_args([])
        assert args.lambda_render == 0.0 and args.render_size == 32
        args = parser.parse_args(["--lambda_render", "0.25", "--render_size", "16"])
        assert args.lambda_render == 0.25 and args.render_size == 16
        assert networks.render_options(args) == {"lambda_render": 0.25, "render_size": 16}
        for bad in ("-0.5", "nan", "much"):
            with pytest.raises(SystemExit):
                parser.parse_args(["--lambda_render", bad])
    capsys.readouterr()
    # the projector's train parser hands them on to the networks' options
    args = options.train_parser().parse_args(["--lambda_render", "2", "--render_size", "24"])
    opt = options.network_options(args, True)
    assert (opt.lambda_render, opt.render_size) == (2.0, 24)
    opt = options.network_options(options.train_parser().parse_args([]), True)
    assert (opt.lambda_render, opt.render_size) == (0.0, 32)
