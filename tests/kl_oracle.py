"""CPU restatement of the KL first stage: ``DiagonalGaussianDistribution``
(latent-diffusion/ldm/modules/distributions/distributions.py:24-62) and ``AutoencoderKL.encode`` / ``decode`` / ``forward``
(latent-diffusion/ldm/models/autoencoder.py:374-393) over oracle/vae_oracle.py's Encoder / Decoder.  Pinned to the
reference by tests/test_kl_host.py against tests/golden/kl.pt; evaluated in fp64 it is what the operator tests compare
the posterior kernel with."""
import math

import torch
import torch.nn.functional as F

from oracle import vae_oracle as vo


class Posterior:
    """distributions.py:24-36 in ``dtype`` (the tensors keep the reference's names)."""

    def __init__(self, parameters, dtype=None):
        self.parameters = parameters if dtype is None else parameters.to(dtype)
        self.mean, logvar = torch.chunk(self.parameters, 2, dim=1)
        self.logvar = torch.clamp(logvar, -30.0, 20.0)
        self.std = torch.exp(0.5 * self.logvar)
        self.var = torch.exp(self.logvar)

    def sample(self, eps):
        """:34-36 with the draw injected."""
        return self.mean + self.std * eps.to(self.mean.dtype)

    def mode(self):
        return self.mean

    def kl(self, other=None):
        """:38-52."""
        if other is None:
            return 0.5 * torch.sum(torch.pow(self.mean, 2) + self.var - 1.0 - self.logvar, dim=[1, 2, 3])
        return 0.5 * torch.sum(torch.pow(self.mean - other.mean, 2) / other.var + self.var / other.var - 1.0 - self.logvar
                               + other.logvar, dim=[1, 2, 3])

    def nll(self, sample, dims=(1, 2, 3)):
        """:54-60."""
        return 0.5 * torch.sum(math.log(2.0 * math.pi) + self.logvar
                               + torch.pow(sample.to(self.mean.dtype) - self.mean, 2) / self.var, dim=list(dims))


def kl_moments(sd, ecfg, x):
    """autoencoder.py:374-376: Encoder -> quant_conv, the posterior's ``parameters``."""
    return F.conv2d(vo.encoder_forward(sd, ecfg, x), sd["quant_conv.weight"], sd["quant_conv.bias"])


def kl_encode(sd, ecfg, x):
    return Posterior(kl_moments(sd, ecfg, x))


def kl_decode(sd, dcfg, z):
    """autoencoder.py:380-383 (the same two steps as VQModel.decode)."""
    return vo.vq_decode(sd, dcfg, z)


def kl_forward(sd, ecfg, dcfg, x, eps=None):
    """autoencoder.py:385-392: ``eps=None`` is ``sample_posterior=False``."""
    posterior = kl_encode(sd, ecfg, x)
    z = posterior.mode() if eps is None else posterior.sample(eps)
    return kl_decode(sd, dcfg, z), posterior
