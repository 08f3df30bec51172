"""CPU: the oracle reproduces the reference's 64-wide-head goldens (tests/golden/make_golden_dim_head.py -> dim_head.pt), so
the GPU tests of tests/test_hip_dim_head.py compare against data the oracle also explains."""
import torch

import diffusion_models_amd as dm
from diffusion_models_amd.spec import UnetConfig
from oracle import unet_oracle as uo

from conftest import load_golden, rel_l2

TOL = 1e-5


def test_oracle_reproduces_dim_head_goldens():
    g = load_golden("dim_head.pt")
    assert g["dim_head"] == 64
    cases = (("unet_a16", dict(dim=32, dim_mults=(1, 2, 4))),
             ("stage_heads", dict(dim=32, dim_mults=(1, 2, 4), attn_heads=(2, 4, 8))),
             ("text_cross", dict(dim=32, dim_mults=(1, 2), text_condition=True, use_cross_attn=True)),
             ("text_cross_m3", dict(dim=32, dim_mults=(1, 2), text_condition=True, use_cross_attn=True)),
             ("text_concat", dict(dim=32, dim_mults=(1, 2), text_condition=True, use_cross_attn=False)))
    for key, kw in cases:
        b = g[key]
        cfg = UnetConfig(channels=3, attn_dim_head=64, **kw)
        sd = dm.synth_state_dict(dm.unet_param_spec(cfg), salt=b["salt"])
        with torch.inference_mode():
            y = uo.unet_forward(sd, cfg, b["x"], b["t"], text_emb=b.get("ctx"))
        err = rel_l2(y, b["y"])
        print(key, f"{err:.3e}")
        assert err < TOL, (key, err)
