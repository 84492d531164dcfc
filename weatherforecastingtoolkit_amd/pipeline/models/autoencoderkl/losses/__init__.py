"""Drop-in for the pieces of `pipeline/models/autoencoderkl/losses/` the AE+GAN step uses
(SURVEY.md §8(f) next-2): PatchGAN discriminator, its initialiser, the hinge loss and the LPIPS
perceptual loss (lpips.py: nothing is fetched, the user supplies the weight files)."""
from .model import NLayerDiscriminator, weights_init  # noqa: F401
from .contperceptual import hinge_d_loss, adopt_weight, LPIPS  # noqa: F401
