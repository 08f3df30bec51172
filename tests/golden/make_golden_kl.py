#!/usr/bin/env python3
"""Golden vectors for the KL first stage (latent-diffusion/ldm/models/autoencoder.py:339-396), generated from the
reference's own ``Encoder`` / ``Decoder`` (as make_golden_encoder.py does) and its own ``DiagonalGaussianDistribution``
(ldm/modules/distributions/distributions.py:24-62); both import here.

    python tests/golden/make_golden_kl.py      ->  tests/golden/kl.pt
``AutoencoderKL`` itself is a LightningModule and pytorch_lightning is absent, so the six lines of its ``encode`` /
``decode`` / ``forward`` (:374-393) are assembled from those parts and two ``torch.nn.Conv2d`` (:356-357), as is done
for ``VQModel``.  Weights are name-seeded (diffusion_models_amd.synth), so only inputs, outputs and the key list are
stored.  ``eps`` is what ``posterior.sample()`` draws from torch's global generator under the case's seed."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

import diffusion_models_amd as dm  # noqa: E402
from diffusion_models_amd.spec import DecoderConfig, EncoderConfig, decoder_param_spec, encoder_param_spec  # noqa: E402

# name -> (ddconfig, embed_dim, weight salt, input shape, seed of the posterior draw)
CASES = {
    "kl_c64": (dict(double_z=True, z_channels=3, resolution=32, in_channels=3, out_ch=3, ch=64, ch_mult=(1, 2),
                    num_res_blocks=2, attn_resolutions=(16,), dropout=0.0), 3, 21, (2, 3, 32, 32), 101),
    "kl_c32_attn8": (dict(double_z=True, z_channels=4, resolution=32, in_channels=3, out_ch=3, ch=32, ch_mult=(1, 2, 4),
                          num_res_blocks=1, attn_resolutions=(8,), dropout=0.0), 4, 22, (2, 3, 32, 32), 102),
}


def configs(ddconfig, embed_dim):
    kw = dict(ch=ddconfig["ch"], ch_mult=tuple(ddconfig["ch_mult"]), num_res_blocks=ddconfig["num_res_blocks"],
              attn_resolutions=tuple(ddconfig["attn_resolutions"]), resolution=ddconfig["resolution"],
              z_channels=ddconfig["z_channels"], embed_dim=embed_dim)
    return (EncoderConfig(in_channels=ddconfig["in_channels"], n_embed=0, double_z=True, **kw),
            DecoderConfig(out_ch=ddconfig["out_ch"], **kw))


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    _, _, ldm_model = mg.import_reference()
    from ldm.modules.distributions.distributions import DiagonalGaussianDistribution

    out = {}
    for name, (ddconfig, embed_dim, salt, shape, draw_seed) in CASES.items():
        ecfg, dcfg = configs(ddconfig, embed_dim)
        ae = torch.nn.Module()  # the attribute order of AutoencoderKL.__init__ (:351-357) without the loss
        ae.encoder = ldm_model.Encoder(**ddconfig)
        ae.decoder = ldm_model.Decoder(**ddconfig)
        assert ddconfig["double_z"]
        ae.quant_conv = torch.nn.Conv2d(2 * ddconfig["z_channels"], 2 * embed_dim, 1)
        ae.post_quant_conv = torch.nn.Conv2d(embed_dim, ddconfig["z_channels"], 1)
        ae.eval()
        sd = dm.synth_state_dict(encoder_param_spec(ecfg) + decoder_param_spec(dcfg), salt=salt)
        keys = list(ae.state_dict())
        assert sorted(keys) == sorted(sd), "parameter names differ from the spec"
        ae.load_state_dict(sd, strict=True)
        x = mg.seeded(shape, 80 + salt)
        with torch.inference_mode():
            moments = ae.quant_conv(ae.encoder(x))                      # encode, :374-378
            posterior = DiagonalGaussianDistribution(moments)
            torch.manual_seed(draw_seed)
            eps = torch.randn(posterior.mean.shape)
            torch.manual_seed(draw_seed)
            z = posterior.sample()
            assert torch.equal(z, posterior.mean + posterior.std * eps)
            mode = posterior.mode()
            dec = ae.decoder(ae.post_quant_conv(z))                      # decode, :380-383
            dec_mode = ae.decoder(ae.post_quant_conv(mode))              # forward(sample_posterior=False)[0], :385-392
            raw = moments[:, embed_dim:]
            inside = float(((raw > -30.0) & (raw < 20.0)).double().mean())
            assert inside >= 0.9, f"{name}: only {inside:.1%} of logvar inside the clamp: the model test would not see the open branch"
            out[name] = dict(x=x, moments=moments.clone(), eps=eps, z=z, mode=mode.clone(), kl=posterior.kl(),
                             nll=posterior.nll(z), dec=dec, dec_mode=dec_mode, keys=keys)
        print(f"{name}: logvar in [{float(raw.min()):.3f}, {float(raw.max()):.3f}], {inside:.1%} inside the clamp, "
              f"|mean| <= {float(posterior.mean.abs().max()):.3f}, kl {posterior.kl().tolist()}")
    mg.save("kl.pt", out)


if __name__ == "__main__":
    main()
