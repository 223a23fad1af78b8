# Opt-in shim for `from edgeconnect.loss import PerceptualLoss, StyleLoss` (the reference's edgeconnect/models.py and its
# evaluation scripts).  By default this module IS the reference's own loss.py (loaded from the checkout further down the merged
# package's path, `FUSG_DROPIN` False): the default alias set does not change.  FUSG_DROPIN_LOSSES=1 selects the device
# versions (csrc/perceptual.hip: forward only - no gradients, AdversarialLoss raises, AdversarialScore computes its values - so never for a training script).
import os as _os

if _os.environ.get("FUSG_DROPIN_LOSSES") == "1":
    from future_urban_scene_generation_amd.edgeconnect.loss import *  # noqa: F401,F403
    from future_urban_scene_generation_amd.edgeconnect.loss import (VGG19, AdversarialLoss, AdversarialScore,  # noqa: F401
                                                                    PerceptualLoss, StyleLoss, feature_distances,
                                                                    feature_matching)
    FUSG_DROPIN = True
else:
    from future_urban_scene_generation_amd._shim import become_reference_module as _become
    _become(__name__, __file__)
