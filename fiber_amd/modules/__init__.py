from .fiber_module import FIBERTransformerSS  # noqa: F401  (reference: fiber/modules/__init__.py:1)
from .vldyhead import TokenSigmoidFocalLoss, VLDyHead  # noqa: F401  (reference: fine_grained/maskrcnn_benchmark/modeling/rpn/vldyhead.py, layers/sigmoid_focal_loss.py)
