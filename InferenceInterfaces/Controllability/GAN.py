"""Same import path as the reference (InferenceInterfaces/Controllability/GAN.py): ``from InferenceInterfaces.Controllability.GAN
import GanWrapper`` picks up the MI355X-native implementation when this repository is on sys.path."""
import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd.controllable import GanWrapper, inverse_normalize  # noqa: F401
