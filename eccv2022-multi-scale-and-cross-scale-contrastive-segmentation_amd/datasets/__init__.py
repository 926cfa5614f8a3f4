from .synthetic import SyntheticSegmentation
from .augment import AugmentPlanner, DeviceAugment, Plan, apply_plan_torch, network_lut
from .raw import ADE20K, Cityscapes, PascalC, SyntheticRaw, list_collate
