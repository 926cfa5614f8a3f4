from .UPerNet import UPerNet
from .Projector import Projector
from .HRNet import hrnet48, hrnet32, hrnet18, HRNet
from .Swin import SwinTransformer
from .OCR import OCRNet, SpatialGatherModule, ObjectAttentionBlock2D, SpatialOCR_Module
from .ResNet import resnet50, resnet101
from .DeepLabv3 import DeepLabv3, ASPP
from .TTA import TTAWrapper, TTAWrapperCTS, TTAWrapperPC, TTAWrapperSlide
