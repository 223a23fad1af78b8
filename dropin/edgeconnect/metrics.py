# Opt-in shim for `from edgeconnect.metrics import PSNR, EdgeAccuracy` (the reference's edgeconnect/models.py and its
# training / evaluation scripts).  By default this module IS the reference's own metrics.py (loaded from the checkout further
# down the merged package's path, `FUSG_DROPIN` False): the default alias set does not change.  FUSG_DROPIN_METRICS=1 selects
# the device versions (csrc/metrics.hip: exact counts and a float64 sum of squared differences instead of float32 sums).
import os as _os

if _os.environ.get("FUSG_DROPIN_METRICS") == "1":
    from future_urban_scene_generation_amd.edgeconnect.metrics import *  # noqa: F401,F403
    from future_urban_scene_generation_amd.edgeconnect.metrics import PSNR, EdgeAccuracy  # noqa: F401
    FUSG_DROPIN = True
else:
    from future_urban_scene_generation_amd._shim import become_reference_module as _become
    _become(__name__, __file__)
