"""Drop-in surfaces mirroring the reference's ``PretrainedBasnetModel/``: ``model.BASNet`` (eval-mode inference on the device)
and ``RunInference`` (the Oxford-IIIT Pet saliency evaluation, as functions)."""
from .model import BASNet, BasicBlock, RefUnet  # noqa: F401
