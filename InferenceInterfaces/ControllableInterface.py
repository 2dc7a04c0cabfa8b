"""Same import path as the reference (InferenceInterfaces/ControllableInterface.py): scripts such as run_controllable_GUI.py
``from InferenceInterfaces.ControllableInterface import ControllableInterface`` pick up the MI355X-native implementation when this
repository is on sys.path."""
import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd.controllable import ControllableInterface  # noqa: F401
