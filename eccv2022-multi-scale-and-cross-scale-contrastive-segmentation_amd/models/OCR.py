"""OCRNet: HRNet backbone + object-contextual representation head (Yuan et al. 2020) + (multi-scale) projector.

Drop-in for the reference (models/OCR.py): same constructor ``OCRNet(config=graph_dict, experiment=int)``, same config keys
(``backbone``, ``out_stride``, ``align_corners``, ``dropout``, ``pretrained``, ``projector``, ``ms_projector``), same module tree
-- so the state_dict keys and shapes are the reference's for ``hrnet48`` and its checkpoints load with ``strict=True`` -- and the
same outputs ``[interm_up_logits, up_logits, proj_features]`` under ``get_intermediate`` / ``return_features``.

The backbone, convolutions, norms, resizes and the projector are this package's own (models/HRNet.py, models/ops.py,
models/fused_bn.py); the context core -- the soft class gather and the pixel-to-class attention -- runs on libdcl_ocr.so through
models/ops_ocr.py where it applies.

Decisions where the reference cannot be followed ("OCRNet"):
  * ResNet backbones need torchvision, which this package does not depend on: ``NotImplementedError``.
  * ``ObjectAttentionBlock2D(scale > 1)`` reads ``self.align_corners``, which the reference never sets; OCRNet always passes 1.
    ``scale == 1`` only, ``NotImplementedError`` otherwise.
  * HRNet with a single ``projector`` and ``before_context: true`` crashes in the reference (``ms_projector_scales`` unset, the
    backbone returns one tensor); here the projector reads the 720-channel concatenation its ``c_in`` is already set for.
  * with ``ms_projector`` the reference builds the projector twice; once here (the keys are the same).
  * ``backbone`` may also name ``hrnet32`` / ``hrnet18`` (the extension models/HRNet.py makes)."""
import torch
import torch.nn as nn

from ..utils import DATASETS_INFO
from . import ops_ocr
from .HRNet import _FACTORIES
from .Projector import Projector
from .fused_bn import FusedBatchNorm2d, bn_act
from .ops import ConvPackGroup, upsample_bilinear, use_direct_conv1x1, use_direct_conv3x3

__all__ = ['OCRNet', 'SpatialGatherModule', 'ObjectAttentionBlock2D', 'SpatialOCR_Module']

_RESNETS = ['resnet18', 'resnet34', 'resnet50', 'resnet101']


class _Seq(nn.Sequential):
    """nn.Sequential with the reference's indices / keys whose forward hands a norm's ReLU to the norm layer (one fused kernel for
    FusedBatchNorm2d; the reference's ``relu(bn(x))`` for every other norm)."""

    def forward(self, x):
        layers = list(self)
        i = 0
        while i < len(layers):
            m = layers[i]
            if isinstance(m, nn.modules.batchnorm._BatchNorm) and i + 1 < len(layers) and isinstance(layers[i + 1], nn.ReLU):
                x = bn_act(m, x, relu=True)
                i += 2
            else:
                x = m(x)
                i += 1
        return x


class SpatialGatherModule(nn.Module):
    """Class representations: the features averaged with the softmax over the pixels of each class's (scaled) logits."""

    def __init__(self, cls_num=0, scale=1):
        super().__init__()
        self.cls_num = cls_num
        self.scale = scale

    def forward(self, feats, probs):
        # feats [B, C, H, W], probs [B, K, H, W] -> [B, C, K, 1]
        assert probs.size(1) == self.cls_num, (probs.shape, self.cls_num)
        return ops_ocr.gather(feats, probs, self.scale)


class ObjectAttentionBlock2D(nn.Module):
    """Pixel-to-class attention: every pixel's query against the K class keys, the values mixed by the softmax over the classes."""

    def __init__(self, in_channels, key_channels, scale=1, norm=nn.BatchNorm2d, aling_corners=True):
        super().__init__()
        if scale != 1:
            raise NotImplementedError(f'ObjectAttentionBlock2D: scale must be 1, got {scale} (the reference reads an attribute it '
                                      'never sets on that path; OCRNet always passes 1)')
        self.scale = scale
        self.in_channels = in_channels
        self.key_channels = key_channels
        self.relu = nn.ReLU(inplace=True)
        self.norm = norm

        def conv(cin, cout):
            return nn.Conv2d(in_channels=cin, out_channels=cout, kernel_size=1, stride=1, padding=0, bias=False)
        kc = self.key_channels
        self.f_pixel = _Seq(conv(in_channels, kc), norm(kc), self.relu, conv(kc, kc), norm(kc), self.relu)
        self.f_object = _Seq(conv(in_channels, kc), norm(kc), self.relu, conv(kc, kc), norm(kc), self.relu)
        self.f_down = _Seq(conv(in_channels, kc), norm(kc), self.relu)
        self.f_up = _Seq(conv(kc, in_channels), norm(in_channels), self.relu)

    def forward(self, x, proxy):
        # x [B, C, H, W], proxy [B, C, K, 1]
        b, h, w = x.size(0), x.size(2), x.size(3)
        query = self.f_pixel(x).reshape(b, self.key_channels, -1)            # [B, Ck, N]
        key = self.f_object(proxy).reshape(b, self.key_channels, -1)         # [B, Ck, K]
        value = self.f_down(proxy).reshape(b, self.key_channels, -1)         # [B, Ck, K]
        context = ops_ocr.object_attention(query, key, value)               # [B, Ck, N]
        return self.f_up(context.view(b, self.key_channels, h, w))


class SpatialOCR_Module(nn.Module):
    """The OCR module: the object context of every pixel, concatenated with its features and mixed by a 1x1 convolution."""

    def __init__(self, in_channels, key_channels, out_channels, scale=1, dropout=0.0, norm=nn.BatchNorm2d, align_corners=True):
        super().__init__()
        self.relu = nn.ReLU(inplace=True)
        self.object_context_block = ObjectAttentionBlock2D(in_channels, key_channels, scale, norm, align_corners)
        self.conv_bn_dropout = _Seq(nn.Conv2d(2 * in_channels, out_channels, kernel_size=1, padding=0, bias=False),
                                    norm(out_channels), self.relu, nn.Dropout2d(dropout))

    def forward(self, feats, proxy_feats):
        context = self.object_context_block(feats, proxy_feats)
        return self.conv_bn_dropout(torch.cat([context, feats], 1))


class OCRNet(nn.Module):
    eligible_backbones = _RESNETS + ['hrnet48', 'hrnet32', 'hrnet18']

    def __init__(self, config, experiment):
        super().__init__()
        self.config = config
        self.dataset = config['dataset']
        self.backbone_name = config['backbone'] if 'backbone' in config else 'resnet50'
        self.out_stride = config['out_stride'] if 'out_stride' in config else 8
        # fused BN(+ReLU) kernels (models/fused_bn.py); same parameters / state_dict as nn.BatchNorm2d
        self.norm = config['norm'] if 'norm' in config else (FusedBatchNorm2d if config.get('fused_bn', True) else nn.BatchNorm2d)
        assert self.backbone_name in self.eligible_backbones, 'backbone must be in {}'.format(self.eligible_backbones)
        names = DATASETS_INFO[self.dataset].CLASS_INFO[experiment][1]
        self.num_classes = len(names) - 1 if 255 in names.keys() else len(names)
        self.experiment = experiment
        self.align_corners = config['align_corners'] if 'align_corners' in config else True
        self.relu = nn.ReLU(inplace=True)
        self.dropout = config['dropout'] if 'dropout' in config else 0.0
        self.backbone_pretrained = True if 'pretrained' not in config else config['pretrained']
        # if true, forward() returns the up-sampled intermediate logits in front of the final ones
        self.get_intermediate = True
        self.return_all_scales = 'ms_projector' in config
        self._get_backbone()
        self._get_ocr()
        self._get_proj()
        self._use_kernels()

    def _get_backbone(self):
        self.backbone_cutoff = None
        if self.backbone_name in _RESNETS:
            raise NotImplementedError(f'OCRNet: backbone {self.backbone_name} needs torchvision, which this package does not '
                                      'depend on; use hrnet48 (or hrnet32 / hrnet18)')
        self.backbone = _FACTORIES[self.backbone_name](
            self.backbone_pretrained, mixing_layer=True, use_as_backbone=True, return_all_scales=self.return_all_scales,
            align_corners=self.align_corners, dataset=self.dataset, experiment=self.experiment, norm_layer=self.norm)
        self.high_level_channels = sum(self.backbone.stage4_cfg.NUM_CHANNELS)      # 720 for hrnet48
        self.low_level_channels = None

    def _get_ocr(self):
        self.ocr_dim = 512
        self.conv_high_map = _Seq(nn.Conv2d(self.high_level_channels, 512, kernel_size=3, stride=1, padding=1),
                                  self.norm(512), self.relu)
        self.interm_pred_c_in = self.high_level_channels
        self.interm_prediction_head = _Seq(
            nn.Conv2d(self.interm_pred_c_in, 512, kernel_size=3, stride=1, padding=1), self.norm(512), self.relu,
            nn.Dropout2d(self.dropout), nn.Conv2d(512, self.num_classes, kernel_size=1, stride=1, padding=0, bias=True))
        self.spatial_gather = SpatialGatherModule(self.num_classes)
        self.spatial_ocr_head = SpatialOCR_Module(in_channels=512, key_channels=256, out_channels=512, scale=1,
                                                  dropout=self.dropout, norm=self.norm, align_corners=self.align_corners)
        self.conv_out = nn.Conv2d(512, self.num_classes, kernel_size=1, stride=1, bias=True)

    def _get_proj(self):
        if 'projector' in self.config:
            self.return_features = True
            self.use_ms_projector = False
            self.projector_before_context = self.config['projector']['before_context']
            self.config['projector']['c_in'] = self.high_level_channels if self.projector_before_context else self.ocr_dim
            self.projector_model = Projector(config=self.config['projector'])
        elif 'ms_projector' in self.config:
            self.return_features = True
            self.use_ms_projector = True
            self.projector_before_context = True       # the multi-scale projector reads the backbone's branches
            self.ms_projector_scales = 4
            self.config['ms_projector']['c_in'] = self.backbone.stage4_cfg.NUM_CHANNELS[:self.ms_projector_scales]
            self.projector_model = Projector(config=self.config['ms_projector'])
        else:
            self.use_ms_projector = False
            self.projector_before_context = None
            self.projector_model = None
            self.return_features = False

    def _use_kernels(self):
        """As HRNet.__init__: the 3x3 and 1x1 convolutions on the direct split-f16 kernels (DirectConv2d decides per input whether
        it takes it), the projector's norms fused, all weights packed by one ConvPackGroup.  The backbone's concatenation stays
        materialised (``lazy_concat`` off): two separate 3x3 convolutions read it."""
        cfg = self.config
        self.backbone.lazy_concat = False
        self._conv_packs = None
        if cfg.get('fused_bn', True) and 'norm' not in cfg and self.projector_model is not None:
            for m in self.projector_model.modules():
                if type(m) is nn.BatchNorm2d:
                    m.__class__ = FusedBatchNorm2d
        self.branch_conv = cfg.get('branch_conv', 'f16x3')
        self.head_conv = cfg.get('head_conv', 'direct')
        self.conv1x1 = cfg.get('conv1x1', 'f16x3')
        if self.branch_conv == 'f16x3':
            use_direct_conv3x3(self.backbone)
        if self.head_conv == 'direct':
            use_direct_conv3x3(self.conv_high_map)
            use_direct_conv3x3(self.interm_prediction_head)
        if self.conv1x1 == 'f16x3':
            use_direct_conv1x1(self)
        if self.branch_conv == 'f16x3' or self.head_conv == 'direct' or self.conv1x1 == 'f16x3':
            self._conv_packs = ConvPackGroup(self)

    def forward(self, x):
        input_resolution = x.shape[-2:]
        if self._conv_packs is not None and x.is_cuda:
            self._conv_packs.refresh()
        backbone_features = self.backbone(x)
        cat = backbone_features[0] if isinstance(backbone_features, (list, tuple)) else backbone_features
        intermediate_logits = self.interm_prediction_head(cat)
        x_high = self.conv_high_map(cat)
        object_global_representation = self.spatial_gather(x_high, intermediate_logits)
        ocr_representation = self.spatial_ocr_head(x_high, object_global_representation)
        logits = self.conv_out(ocr_representation)
        up_logits = upsample_bilinear(logits, input_resolution, self.align_corners)

        outputs = []        # the order is [interm_up_logits (optional), up_logits, proj_feats (optional)]
        if self.get_intermediate:
            outputs.append(upsample_bilinear(intermediate_logits, input_resolution, self.align_corners))
        outputs.append(up_logits)
        if self.projector_model:
            if self.use_ms_projector:
                proj_features = self.projector_model(backbone_features[1][:self.ms_projector_scales])
            elif self.projector_before_context:
                proj_features = self.projector_model(cat)
            else:
                proj_features = self.projector_model(ocr_representation)
            if self.return_features:
                outputs.append(proj_features)
        if not self.get_intermediate and not self.return_features:
            assert len(outputs) == 1
            return outputs[0]
        return outputs
