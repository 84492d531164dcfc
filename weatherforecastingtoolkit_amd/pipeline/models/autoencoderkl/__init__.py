from .autoencoder_kl import AutoencoderKL  # noqa: F401
from .distributions import DiagonalGaussianDistribution  # noqa: F401
