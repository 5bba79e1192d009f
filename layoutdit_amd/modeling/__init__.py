from .dit_backbone import DiTBackbone  # noqa: F401
from .dit_encoder import DiTEncoder, DiTEncoderOutput  # noqa: F401
from .dit_fpn import DiTWithFPN  # noqa: F401
from .detector_input import DetectorInputTransform, ImageList  # noqa: F401
from .rpn import AnchorGenerator, RPNHead, RegionProposalNetwork  # noqa: F401
from .roi_heads import FastRCNNPredictor, MultiScaleRoIAlign, RoIHeads, TwoMLPHead  # noqa: F401
from .detector import LayoutDetectionModel  # noqa: F401
