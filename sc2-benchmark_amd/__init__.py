"""sc2bench_amd: MI355X-native implementation of sc2bench's supervised-compression bottleneck path.

The directory is named ``sc2-benchmark_amd`` (not an importable identifier); ``sc2bench_amd.py`` at the
repository root loads it under the module name ``sc2bench_amd``.
"""
from . import hip  # noqa: F401
from .analysis import ANALYZER_CLASS_DICT, AnalyzableModule, FileSizeAccumulator, FileSizeAnalyzer  # noqa: F401
from .backbone import (BACKBONE_CLASS_DICT, BACKBONE_FUNC_DICT, MODEL_DICT, FeatureExtractionBackbone,  # noqa: F401
                       SplittableResNet, UpdatableBackbone, check_if_updatable, custom_resnet50, get_backbone, splittable_resnet)
from .entropy import (CompressionModel, EntropyBottleneck, GDN1, GaussianConditional, HipConv2d,  # noqa: F401
                      HipConvTranspose2d, LowerBound, NonNegativeParametrizer, get_scale_table)
from .layer import (LAYER_CLASS_DICT, LAYER_FUNC_DICT, BaseBottleneck, EntropyBottleneckLayer,  # noqa: F401
                    FPBasedResNetBottleneck, MSHPBasedResNetBottleneck, SHPBasedResNetBottleneck, SimpleBottleneck, get_layer,
                    larger_resnet_bottleneck, register_layer_class, register_layer_func)
from .loss import BppLoss  # noqa: F401
from . import detection  # noqa: F401
from .detection import (AnchorGenerator, FastRCNNPredictor, FasterRCNN, GeneralizedRCNNTransform, ImageList,  # noqa: F401
                        MultiScaleRoIAlign, RegionProposalNetwork, RoIHeads, RPNHead, TwoMLPHead, batched_nms,
                        multiscale_roi_align, nms, roi_align)
from .compression import (COMPRESSION_MODEL_CLASS_DICT, COMPRESSION_MODEL_FUNC_DICT, FactorizedPrior,  # noqa: F401
                          JointAutoregressiveHierarchicalPriors, MeanScaleHyperprior, ScaleHyperprior,
                          bmshj2018_factorized, bmshj2018_hyperprior, get_compression_model, mbt2018, mbt2018_mean)
from .entropy import GDN  # noqa: F401
from .transforms import (AdaptivePad, PILImageModule, PILTensorModule, QuantizedTensor, SimpleDequantizer,  # noqa: F401
                         SimpleQuantizer, cat_list, coco_collate_fn, dequantize_tensor, pascal_seg_collate_fn, pascal_seg_eval_collate_fn,
                         quantize_tensor)
from .detection import RCNNTransformWithCompression  # noqa: F401
from .wrapper import (WRAPPER_CLASS_DICT, CodecFeatureCompressionClassifier, CodecInputCompressionClassifier,  # noqa: F401
                      CodecInputCompressionSegmentationModel, EntropicClassifier, InputCompressionDetectionModel,
                      NeuralInputCompressionClassifier, SplitClassifier, get_wrapped_detection_model,
                      get_wrapped_segmentation_model, load_detection_model, load_segmentation_model, wrap_model)

from .dense import (DETECTION_MODEL_FUNC_DICT, SEGMENTATION_MODEL_FUNC_DICT, BaseRCNN, BaseSegmentationModel,  # noqa: F401
                    ResizedLogits, SegEvaluator, UpdatableBackboneWithFPN, backbone_with_fpn, deeplabv3_model, deeplabv3_resnet50,
                    faster_rcnn_model, fasterrcnn_resnet50_fpn, seg_cross_entropy, seg_labels)

from . import coco_eval  # noqa: F401
from .coco_eval import CocoBoxEvaluator, CocoDictDetection, coco_gt_from_dataset  # noqa: F401
from . import coco_data  # noqa: F401
from .coco_data import GroupedBatchSampler, coco_dataset, create_aspect_ratio_groups  # noqa: F401
from .transforms import DeferredDetBatch, DeferredDetSample  # noqa: F401
from .pipeline import StagePipeline, supports_stages  # noqa: F401
from . import graphs  # noqa: F401

__version__ = '0.3.0'
