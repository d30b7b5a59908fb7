from .fiber_module import FIBERTransformerSS  # noqa: F401  (reference: fiber/modules/__init__.py:1)
from .vldyhead import TokenSigmoidFocalLoss, VLDyHead  # noqa: F401  (reference: fine_grained/maskrcnn_benchmark/modeling/rpn/vldyhead.py, layers/sigmoid_focal_loss.py)
from .grounding_inference import (ATSSPostProcessor, AnchorGenerator, BoxCoder, Detections, VLDyHeadModule,  # noqa: F401  (reference: modeling/rpn/inference.py, anchor_generator.py, box_coder.py, vldyhead.py:917-1155)
                                  make_anchor_generator_complex, make_atss_postprocessor)
