"""Same import path as the reference (InferenceInterfaces/UtteranceCloner.py): scripts such as run_prosody_override.py
``from InferenceInterfaces.UtteranceCloner import UtteranceCloner`` pick up the MI355X-native implementation when this repository
is on sys.path."""
import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd.cloner import UtteranceCloner  # noqa: F401
