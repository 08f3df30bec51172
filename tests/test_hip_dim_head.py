"""64-wide attention heads (Unet(attn_dim_head=64)): the operators against the oracle, the model against the reference's
goldens (tests/golden/make_golden_dim_head.py -> dim_head.pt), graph and batch invariance, one training iteration with a
checkpoint round trip, the refusals, and every dispatch switch in a child process."""
import os
import subprocess
import sys

import pytest
import torch

import diffusion_models_amd as dm
from diffusion_models_amd import _lib
from diffusion_models_amd.spec import UnetConfig
from oracle import sampler_oracle as so
from oracle import unet_oracle as uo

from conftest import check_grad_digest, load_golden, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DH = 64
OP_TOL = 2e-5     # the operator files' tolerance
FWD_TOL = 1e-5    # model forward against the reference
LOOP_TOL = 2e-5   # DDIM / DDPM loops
GRAD_TOL = 2e-4   # gradient digests, as test_hip_model.py's per-stage-heads test


@pytest.fixture(scope="module")
def golden():
    return load_golden("dim_head.pt")


def seeded(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def dev(t):
    return t.detach().to(DEV).contiguous()


def _attn_params(C, heads, full, seed):
    hid = heads * DH
    sd = {"a.norm.g": 1 + 0.25 * seeded((1, C, 1, 1), seed),
          "a.mem_kv": seeded((2, heads, 4, DH) if full else (2, heads, DH, 4), seed + 1),
          "a.to_qkv.weight": seeded((3 * hid, C, 1, 1), seed + 2) / C ** 0.5}
    if full:
        sd["a.to_out.weight"] = seeded((C, hid, 1, 1), seed + 3) / hid ** 0.5
        sd["a.to_out.bias"] = seeded((C,), seed + 4, 0.1)
    else:
        sd["a.to_out.0.weight"] = seeded((C, hid, 1, 1), seed + 3) / hid ** 0.5
        sd["a.to_out.0.bias"] = seeded((C,), seed + 4, 0.1)
        sd["a.to_out.1.g"] = 1 + 0.25 * seeded((1, C, 1, 1), seed + 5)
    return {k: v.requires_grad_(True) for k, v in sd.items()}


# C = 64 / 128 take the fused LinearAttention at width 32 and the unfused chain here; 4x4 maps with C >= 256 take attn16 at 32;
# 32x32 and 64x64 maps: 1024 / 4096 tokens (16 waves per context); odd maps; over 320 tokens the tiled softmax core
LIN_CASES = [(2, 64, 32, 32, 4), (2, 128, 16, 16, 8), (3, 256, 8, 8, 1), (2, 256, 4, 4, 4), (2, 32, 5, 7, 4),
             (1, 64, 64, 64, 1), (2, 128, 9, 13, 8)]
FULL_CASES = [(2, 256, 4, 4, 4), (3, 512, 4, 4, 8), (2, 512, 8, 8, 1), (2, 64, 3, 5, 4), (1, 128, 16, 16, 4),
              (2, 64, 1, 1, 8), (1, 64, 32, 16, 4), (2, 32, 23, 25, 1)]


@pytest.mark.parametrize("case", LIN_CASES)
def test_linear_attention_op_dh64(case):
    B, C, H, W, heads = case
    sd = _attn_params(C, heads, False, 10)
    x = seeded((B, C, H, W), 1).requires_grad_(True)
    y = uo.linear_attention(sd, "a", x, heads, DH)
    names = ["a.norm.g", "a.mem_kv", "a.to_qkv.weight", "a.to_out.0.weight", "a.to_out.0.bias", "a.to_out.1.g"]
    lib = _lib.load()
    out = torch.empty((B, C, H, W), device=DEV)
    ins = [dev(x)] + [dev(sd[k]) for k in names]
    _lib.check(lib.dm_op_linear_attention(*[_lib.ptr(t) for t in ins], _lib.ptr(out), B, C, H, W, heads, DH, None))
    errs = {"fwd": rel_l2(out.cpu(), y.detach())}
    dy = seeded(tuple(y.shape), 2)
    y.backward(dy)
    dx = torch.empty(x.shape, device=DEV)
    outs = [torch.empty(sd[k].shape, device=DEV) for k in names]
    _lib.check(lib.dm_op_linear_attention_bwd(*[_lib.ptr(t) for t in ins + [dev(dy)]], _lib.ptr(dx),
                                              *[_lib.ptr(t) for t in outs], B, C, H, W, heads, DH, None))
    errs["dx"] = rel_l2(dx.cpu(), x.grad)
    errs.update({k: rel_l2(o.cpu(), sd[k].grad) for k, o in zip(names, outs)})
    print(case, {k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) < OP_TOL, errs


@pytest.mark.parametrize("case", FULL_CASES)
def test_attention_op_dh64(case):
    B, C, H, W, heads = case
    sd = _attn_params(C, heads, True, 20)
    x = seeded((B, C, H, W), 1).requires_grad_(True)
    y = uo.full_attention(sd, "a", x, heads, DH)
    names = ["a.norm.g", "a.mem_kv", "a.to_qkv.weight", "a.to_out.weight", "a.to_out.bias"]
    lib = _lib.load()
    out = torch.empty((B, C, H, W), device=DEV)
    ins = [dev(x)] + [dev(sd[k]) for k in names]
    _lib.check(lib.dm_op_attention(*[_lib.ptr(t) for t in ins], _lib.ptr(out), B, C, H, W, heads, DH, None))
    errs = {"fwd": rel_l2(out.cpu(), y.detach())}
    dy = seeded(tuple(y.shape), 2)
    y.backward(dy)
    dx = torch.empty(x.shape, device=DEV)
    outs = [torch.empty(sd[k].shape, device=DEV) for k in names]
    _lib.check(lib.dm_op_attention_bwd(*[_lib.ptr(t) for t in ins + [dev(dy)]], _lib.ptr(dx), *[_lib.ptr(t) for t in outs],
                                       B, C, H, W, heads, DH, None))
    errs["dx"] = rel_l2(dx.cpu(), x.grad)
    errs.update({k: rel_l2(o.cpu(), sd[k].grad) for k, o in zip(names, outs)})
    print(case, {k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) < OP_TOL, errs


def _unet(salt, **kw):
    cfg = UnetConfig(channels=3, attn_dim_head=DH, **kw)
    u = dm.Unet(channels=3, attn_dim_head=DH, device=DEV, **kw)
    u.load_state_dict(dm.synth_state_dict(dm.unet_param_spec(cfg), salt=salt))
    return u


def unpack(g):
    """make_golden_dim_head.py's packed gradient digests -> {name: check_grad_digest's dict}"""
    heads = torch.split(g["head"], g["head_len"].tolist())
    return {n: dict(norm=float(g["norm"][i]), proj=g["proj"][i], head=heads[i]) for i, n in enumerate(g["names"])}


def _check_train(d, b, text_emb=None):
    kw = {} if text_emb is None else dict(text_emb=text_emb)
    loss = float(d.p_losses(b["img"] * 2 - 1, b["tt"], noise=b["noise"], **kw))
    print("loss", loss, b["loss"], f"rel {abs(loss - b['loss']) / abs(b['loss']):.2e}")
    assert abs(loss - b["loss"]) <= 1e-4 * abs(b["loss"]), (loss, b["loss"])
    grads = d.model.grads()
    worst = 0.0
    for name, dg in unpack(b["grads"]).items():
        g = grads[name].cpu()
        worst = max(worst, abs(float(g.double().norm()) - dg["norm"]) / max(dg["norm"], 1e-30))
        check_grad_digest(name, g, dg, GRAD_TOL)
    print("worst gradient-norm rel error", f"{worst:.2e}")


def test_unet_forward_dh64(golden):
    u = _unet(61, dim=32, dim_mults=(1, 2, 4))
    for key in ("unet_a16", "unet_a32"):
        b = golden[key]
        err = rel_l2(u(b["x"].to(DEV), b["t"].to(DEV)).cpu(), b["y"])
        print(key, f"{err:.3e}")
        assert err < FWD_TOL
    b = golden["unet_bench"]
    ub = _unet(62, dim=64, dim_mults=(1, 2, 4, 8))
    err = rel_l2(ub(b["x"].to(DEV), b["t"].to(DEV)).cpu(), b["y"])
    print("unet_bench", f"{err:.3e}")
    assert err < FWD_TOL


def test_unet_loss_and_gradients_dh64(golden):
    u = _unet(61, dim=32, dim_mults=(1, 2, 4))
    _check_train(dm.DenoisingDiffusion(u, image_size=16, timesteps=1000).train(), golden["train_a16"])
    b = golden["stage_heads"]
    uh = _unet(63, dim=32, dim_mults=(1, 2, 4), attn_heads=(2, 4, 8))
    err = rel_l2(uh(b["x"].to(DEV), b["t"].to(DEV)).cpu(), b["y"])
    print("stage_heads forward", f"{err:.3e}")
    assert err < FWD_TOL
    _check_train(dm.DenoisingDiffusion(uh, image_size=16, timesteps=1000).train(), b)


def test_text_unets_dh64(golden):
    u = _unet(64, dim=32, dim_mults=(1, 2), text_condition=True, use_cross_attn=True)
    for key in ("text_cross", "text_cross_m3"):
        b = golden[key]
        err = rel_l2(u(b["x"], b["t"], text_emb=b["ctx"]).cpu(), b["y"])
        print(key, f"{err:.3e}")
        assert err < FWD_TOL
    uc = _unet(65, dim=32, dim_mults=(1, 2), text_condition=True, use_cross_attn=False)
    b = golden["text_concat"]
    err = rel_l2(uc(b["x"], b["t"], text_emb=b["ctx"]).cpu(), b["y"])
    print("text_concat", f"{err:.3e}")
    assert err < FWD_TOL
    b = golden["train_text_cross"]
    _check_train(dm.DenoisingDiffusion(u, image_size=16, timesteps=1000).train(), b, text_emb=b["ctx"])


@pytest.mark.parametrize("use_graph", [False, True])
def test_samplers_dh64(golden, use_graph):
    u = _unet(61, dim=32, dim_mults=(1, 2, 4))
    d = dm.DenoisingDiffusion(u, image_size=16, timesteps=1000, use_graph=use_graph)
    b = golden["ddim20"]
    y = d.ddim_sample(b["shape"], sampling_timesteps=b["S"], noise=so.NoiseStream(b["seed"])).cpu()
    err = rel_l2(y, b["y"])
    print("ddim20", use_graph, f"{err:.3e}")
    assert err < LOOP_TOL
    b = golden["ddpm50"]
    d50 = dm.DenoisingDiffusion(u, image_size=16, timesteps=b["T"], use_graph=use_graph)
    y = d50.p_sample_loop(b["shape"], noise=so.NoiseStream(b["seed"])).cpu()
    err = rel_l2(y, b["y"])
    print("ddpm50", use_graph, f"{err:.3e}")
    assert err < LOOP_TOL


class PerImageNoise:
    """Injected sampler noise whose image i of draw k does not depend on the batch size."""

    def __init__(self, seed):
        self.seed, self.k = seed, 0

    def __call__(self, shape):
        self.k += 1
        return torch.stack([seeded(tuple(shape[1:]), self.seed * 100003 + self.k * 1009 + i) for i in range(shape[0])])


def test_graph_once_per_shape_and_batch_invariance_dh64():
    """The step graph is captured once per shape; the first 4 images of a B = 8 seeded DDIM run equal a B = 4 run bit for
    bit (the waves per (image, head) of the context kernel depend on the sequence length alone)."""
    u = _unet(62, dim=64, dim_mults=(1, 2, 4, 8))
    d = dm.DenoisingDiffusion(u, image_size=32, timesteps=1000, sampling_timesteps=4)
    a = d.sample(batch_size=4, seed=1)
    n0 = u.graph_captures
    outs = [d.sample(batch_size=4, seed=s) for s in (2, 1)]
    assert u.graph_captures == n0
    assert torch.equal(outs[1], a) and not torch.equal(outs[0], a)
    noise = so.NoiseStream(7)
    y8 = d.ddim_sample((8, 3, 32, 32), sampling_timesteps=4, noise=noise).cpu()
    assert u.graph_captures == n0 + 1
    g = torch.Generator().manual_seed(3)
    x8 = torch.randn((8, 3, 32, 32), generator=g)
    t8 = torch.full((8,), 500, dtype=torch.long)
    f8 = u(x8.to(DEV), t8.to(DEV)).cpu()
    f4 = u(x8[:4].to(DEV), t8[:4].to(DEV)).cpu()
    assert torch.equal(f8[:4], f4)
    s8 = d.ddim_sample((8, 3, 32, 32), sampling_timesteps=4, noise=PerImageNoise(11)).cpu()
    s4 = d.ddim_sample((4, 3, 32, 32), sampling_timesteps=4, noise=PerImageNoise(11)).cpu()
    assert bool(torch.isfinite(y8).all())
    assert torch.equal(s8[:4], s4), float((s8[:4] - s4).abs().max())


def test_training_iteration_and_checkpoint_dh64(tmp_path):
    """One iteration through train.py (Adam, EMA, state_dict(ema=True)), Trainer.save's layout, reload through
    checkpoint.py into a fresh handle, and a forward of the reloaded model."""
    cfg = dict(dim=32, dim_mults=(1, 2, 4))
    u = _unet(61, **cfg)
    d = dm.DenoisingDiffusion(u, image_size=16, timesteps=1000)
    ema = dm.EMA(d, beta=0.995, update_every=1, update_after_step=0)
    g = torch.Generator().manual_seed(5)
    before = {k: v.clone() for k, v in d.model.state_dict().items()}
    dm.train_step(d, [torch.rand((4, 3, 16, 16), generator=g)], lr=1e-3, ema=ema)
    after = d.model.state_dict()
    assert any(not torch.equal(before[k], after[k]) for k in before)
    e = d.model.state_dict(ema=True)
    assert e.keys() == after.keys() and all(bool(torch.isfinite(v).all()) for v in e.values())
    path = tmp_path / "model-1.pt"
    dm.save_checkpoint(path, d, step=1, ema=ema, lr=1e-3)
    data = torch.load(str(path), map_location="cpu", weights_only=True)
    mem = [v for k, v in data["model"].items() if k.endswith("mem_kv")]
    assert mem and all(DH in tuple(v.shape) for v in mem)
    d.model.sync()
    u2 = _unet(0, **cfg)
    d2 = dm.DenoisingDiffusion(u2, image_size=16, timesteps=1000)
    ema2 = dm.EMA(d2, beta=0.995, update_every=1, update_after_step=0)
    step, _ = dm.load_checkpoint(path, d2, ema=ema2)
    assert step == 1
    x = seeded((2, 3, 16, 16), 9)
    t = torch.tensor([10, 900])
    a = d.model(x.to(DEV), t.to(DEV)).cpu()
    b = d2.model(x.to(DEV), t.to(DEV)).cpu()
    assert torch.equal(a, b)


def test_refusals():
    for bad in (48, 16):
        with pytest.raises(Exception, match="32 and 64"):
            dm.Unet(dim=32, dim_mults=(1, 2), attn_dim_head=bad, device=DEV)
    with pytest.raises(NotImplementedError, match="32 and 64"):
        dm.Unet(dim=32, dim_mults=(1, 2, 4), attn_dim_head=(64, 32, 64), device=DEV)
    u = dm.Unet(dim=32, dim_mults=(1, 2, 4), attn_dim_head=(64, 64, 64), device=DEV)
    assert u.cfg.attn_dim_head == DH


SWITCH_SETS = [
    dict(DM_NO_FUSED_LINATTN="1", DM_NO_ATTN16="1", DM_ATTN_TILED="1"),
    dict(DM_ATTN_BWD_TILED="1"),
    dict(DM_ATTN_BWD_NO_CACHE="1"),
]


def test_forced_routes_dh64():
    """The operator and model cases above under every dispatch switch, one child process per switch set (the switches are
    read once per process)."""
    for extra in SWITCH_SETS:
        env = dict(os.environ, **extra)
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k",
                            "op_dh64 or forward_dh64 or loss_and_gradients_dh64 or text_unets_dh64", "-p",
                            "no:cacheprovider"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, (extra, r.stdout[-4000:] + r.stderr[-2000:])
