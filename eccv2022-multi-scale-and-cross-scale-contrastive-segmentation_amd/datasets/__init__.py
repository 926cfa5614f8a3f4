from .synthetic import SyntheticSegmentation
from .augment import AugmentPlanner, ChainPlanner, DeviceAugment, Plan, apply_plan_torch, network_lut, planner_for
from .raw import ADE20K, CaDIS, Cityscapes, PascalC, SyntheticRaw, list_collate, read_frame_table
