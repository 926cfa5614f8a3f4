"""DeepLabv3: a dilated ResNet-50 / ResNet-101 (models/ResNet.py), Atrous Spatial Pyramid Pooling and a 1x1 classifier, with the
config keys (``backbone``, ``aspp.channels``, ``out_stride``, ``align_corners``, ``pretrained``, ``projector``, ``ms_projector`` with
``feats``), module names (``backbone.*``, ``aspp.aspp1..5``, ``aspp.aspp1_bn..5_bn``, ``aspp.conv2``, ``aspp.bn2``, ``conv_out``,
``projector_model``) and return values (``upsampled_logits`` or ``(upsampled_logits, proj_features)``) of the reference's
models/DeepLabv3.py.

Kept from the reference on purpose:
  * ASPP builds its norms as ``norm(c_aspp, momentum)``: the second positional argument of a BatchNorm is ``eps``, so 0.0003 is
    the norms' eps and their momentum stays 0.1.
  * the logits are up-sampled with ``align_corners=True`` whatever the config says; ``align_corners`` reaches only the ASPP.
  * the multi-scale projector reads 256 channels for its first map whichever layer ``feats`` names first (the reference tests
    the torchvision name against a list of paper names), 1024 for a middle one.
  * ``resnet18`` is listed but never built: ``NotImplementedError``.

Kernels: the dilated 3x3 convolutions (ASPP branches 2..4, the ResNet layers whose stride became dilation) run on libdcl_dconv.so
(models/ops_dconv.py), the 1x1 and undilated 3x3 ones on DirectConv2d; the norms are FusedBatchNorm2d and are never deferred.  The
image-level branch's bilinear resize of a 1x1 map is a broadcast (every output pixel interpolates the one value)."""
import torch
import torch.nn as nn

from ..utils import DATASETS_INFO, printlog
from .Projector import Projector
from .ResNet import PAPER_NAMES, resnet50, resnet101
from .fused_bn import FusedBatchNorm2d, bn_act
from .ops import upsample_bilinear, use_direct_conv1x1
from .ops_dconv import use_dilated_conv3x3

_FACTORIES = {'resnet50': resnet50, 'resnet101': resnet101}


class ASPP(nn.Module):
    """Five parallel branches over the same map -- 1x1, three dilated 3x3 (6, 12, 18 times ``mult``) and the image-level average --
    each followed by norm + ReLU, concatenated and mixed by a 1x1 convolution + norm + ReLU."""

    def __init__(self, c_in, c_aspp, conv=nn.Conv2d, norm=nn.BatchNorm2d, momentum=0.0003, mult=1, align_corners=True):
        super().__init__()
        self._c_in, self._c_aspp = c_in, c_aspp
        self.align_corners = align_corners
        self.global_pooling = nn.AdaptiveAvgPool2d(1)
        self.relu = nn.ReLU(inplace=True)
        rates = [int(r * mult) for r in (6, 12, 18)]
        self.aspp1 = conv(c_in, c_aspp, kernel_size=1, stride=1, bias=False)
        for i, r in enumerate(rates):
            setattr(self, f'aspp{i + 2}', conv(c_in, c_aspp, kernel_size=3, stride=1, dilation=r, padding=r, bias=False))
        self.aspp5 = conv(c_in, c_aspp, kernel_size=1, stride=1, bias=False)
        for i in range(1, 6):
            setattr(self, f'aspp{i}_bn', norm(c_aspp, momentum))      # (sic: lands in eps, see the module docstring)
        self.conv2 = conv(c_aspp * 5, c_aspp, kernel_size=1, stride=1, bias=False)
        self.bn2 = norm(c_aspp, momentum)

    def forward(self, x):
        h, w = x.shape[2], x.shape[3]
        branches = [bn_act(getattr(self, f'aspp{i}_bn'), getattr(self, f'aspp{i}')(x)) for i in range(1, 5)]
        pooled = bn_act(self.aspp5_bn, self.aspp5(self.global_pooling(x)))
        branches.append(pooled.expand(-1, -1, h, w))
        return bn_act(self.bn2, self.conv2(torch.cat(branches, 1)))


class DeepLabv3(nn.Module):
    eligible_backbones = ['resnet18', 'resnet50', 'resnet101']

    def __init__(self, config, experiment):
        super().__init__()
        self.config = config
        self.backbone_name = config['backbone'] if 'backbone' in config else 'resnet50'
        self.c_aspp = config['aspp']['channels'] if 'aspp' in config else 256
        self.out_stride = config['out_stride'] if 'out_stride' in config else 16
        self.dataset = config['dataset']
        self.align_corners = config['align_corners'] if 'align_corners' in config else True
        self.norm = config['norm'] if 'norm' in config else (FusedBatchNorm2d if config.get('fused_bn', True) else nn.BatchNorm2d)
        assert self.out_stride in [8, 16, 32]
        assert self.backbone_name in self.eligible_backbones, 'backbone must be in {}'.format(self.eligible_backbones)
        striding = {8: [False, True, True], 16: [False, False, True], 32: [False, False, False]}[self.out_stride]
        names = DATASETS_INFO[self.dataset].CLASS_INFO[experiment][1]
        self.num_classes = len(names) - 1 if 255 in names.keys() else len(names)

        self.use_ms_projector = False
        self.backbone_cutoff = {'layer4': 'C5'}
        self.proj_feats = []
        if 'ms_projector' in config:
            if 'feats' in config['ms_projector']:
                picked = {f: PAPER_NAMES[f] for f in config['ms_projector']['feats']}
            else:
                picked = {'layer1': 'C2'}                       # configs from before the key existed
            self.proj_feats = list(picked.values())
            self.backbone_cutoff.update(picked)

        if self.backbone_name not in _FACTORIES:
            raise NotImplementedError(f'{self.backbone_name}')
        pretrained = True if 'pretrained' not in config else config['pretrained']
        self.backbone = _FACTORIES[self.backbone_name](pretrained=pretrained, replace_stride_with_dilation=striding,
                                                       return_layers=self.backbone_cutoff, norm_layer=self.norm)
        self.backbone_out_channels = self.backbone.layer4[-1].conv3.out_channels

        self.aspp = ASPP(c_in=self.backbone_out_channels, c_aspp=self.c_aspp, norm=self.norm, mult=2, align_corners=self.align_corners)
        self.conv_out = nn.Conv2d(self.c_aspp, self.num_classes, kernel_size=1, stride=1)

        if 'projector' in config:
            self.return_features = True
            self.projector_before_context = config['projector']['before_context']
            self.config['projector']['c_in'] = self.backbone_out_channels if self.projector_before_context else self.c_aspp
            self.projector_model = Projector(config=self.config['projector'])
            printlog('added projector from {} to {}'.format(self.projector_model.c_in, self.projector_model.d))
        elif 'ms_projector' in config:
            self.return_features = True
            self.mid1_channels = 512 if 'layer2' in self.proj_feats else 256       # (sic: proj_feats holds C2 .. C5, so 256)
            self.mid2_channels = 1024
            if len(self.proj_feats) == 2:
                c_in = [self.mid1_channels, self.backbone_out_channels]
            elif len(self.proj_feats) == 3:
                c_in = [self.mid1_channels, self.mid2_channels, self.backbone_out_channels]
            else:
                raise NotImplementedError(f'invalid : {self.proj_feats}')
            self.config['ms_projector']['c_in'] = c_in
            self.projector_model = Projector(config=self.config['ms_projector'])
            printlog('added ms projectors from {} to {}'.format(self.projector_model.c_in, self.projector_model.d))
            self.use_ms_projector = True
            self.projector_before_context = True                # the multi-scale projector reads the backbone's maps
        else:
            self.projector_before_context = None
            self.projector_model = None
            self.return_features = False
        self._use_kernels()

    def _use_kernels(self):
        cfg = self.config
        if cfg.get('fused_bn', True) and 'norm' not in cfg and self.projector_model is not None:
            for m in self.projector_model.modules():
                if type(m) is nn.BatchNorm2d:
                    m.__class__ = FusedBatchNorm2d
        if cfg.get('conv_kernels', True):
            self.backbone.use_kernels()
            use_dilated_conv3x3(self.aspp)
            use_direct_conv1x1(self.aspp)
            use_direct_conv1x1(self.conv_out)
            if self.projector_model is not None:
                use_direct_conv1x1(self.projector_model)

    def forward(self, x):
        input_resolution = x.shape[-2:]
        backbone_features = self.backbone(x)
        aspp_features = self.aspp(backbone_features['C5'])
        logits = self.conv_out(aspp_features)
        upsampled_logits = upsample_bilinear(logits, input_resolution, True)
        if not self.projector_model:
            return upsampled_logits
        if not self.projector_before_context:
            proj_features = self.projector_model(aspp_features)
        elif self.use_ms_projector:
            proj_features = self.projector_model([backbone_features[f] for f in self.proj_feats])
        else:
            proj_features = self.projector_model(backbone_features['C5'])
        return (upsampled_logits, proj_features) if self.return_features else upsampled_logits

    def print_params(self):
        for name, t in self.state_dict().items():
            print(name, "\t", t.size())
