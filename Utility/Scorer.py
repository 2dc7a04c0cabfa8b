"""Same import path as the reference (Utility/Scorer.py): scripts such as run_scorer.py ``from Utility.Scorer import AlignmentScorer,
TTSScorer`` pick up the MI355X-native implementation when this repository is on sys.path."""
import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd.scorer import AlignmentScorer, TTSScorer  # noqa: F401
from ims_toucan_prosody_variance_amd.fidelity import VocoderScorer  # noqa: F401  (additive: the reference has no vocoder scorer)
