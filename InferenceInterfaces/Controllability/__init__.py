"""The reference's ``InferenceInterfaces.Controllability`` package path.  This repository provides ``Controllability.GAN`` only; with the
reference's checkout also on ``sys.path`` its other modules (``Controllability.wgan``, ``Controllability.dataset``) stay importable
from there."""
import pkgutil

__path__ = pkgutil.extend_path(__path__, __name__)
