"""SubmapAlignParams — registration parameters and the `method` -> plugin factory.
Mirrors the registration half of [REF roman/params/submap_align_params.py:25-150] (the IO helper
class SubmapAlignInputOutput is out of scope)."""
from dataclasses import dataclass
from typing import Union

import yaml

from .. import _abi
from .dist_reg_with_pruning import DistRegWithPruning
from .ransac_reg import RansacReg
from .roman_registration import ROMANParams, ROMANRegistration


@dataclass
class SubmapAlignParams:
    # same fields, order and defaults as [REF roman/params/submap_align_params.py:27-74]
    dim: int = 3
    method: str = 'roman'
    fusion_method: str = 'geometric_mean'

    force_fill_submaps: bool = False
    submap_max_size: int = 40
    submap_overlap: int = int(0.5 * 40)
    submap_radius: float = 15.0
    submap_center_dist: float = 10.0
    submap_center_time: float = 50.0
    submap_pruning_method: str = 'distance'
    submap_descriptor: Union[str, None] = None
    frame_descriptor_dist: float = None
    submap_descriptor_thresh: float = 0.8

    single_robot_lc: bool = False
    single_robot_lc_time_thresh: float = 50.0
    force_rm_lc_roll_pitch: bool = True
    force_rm_upside_down: bool = True
    use_object_bottom_middle: bool = False

    sigma: float = 0.4
    epsilon: float = 0.6
    mindist: float = 0.2
    epsilon_shape: float = 0.0
    ransac_iter: int = int(1e6)
    cosine_min: float = 0.5
    cosine_max: float = 0.7
    semantics_dim: int = 768
    gravity_unc_ang_rad: float = 0.0872665

    def __post_init__(self):
        if type(self.submap_descriptor) == str and self.submap_descriptor.lower() == 'none':
            self.submap_descriptor = None

    @classmethod
    def from_yaml(cls, yaml_file):
        with open(yaml_file, 'r') as f:
            params = yaml.full_load(f)
        return cls(**params)

    def get_object_registration(self):
        """`method` string -> registration object, [REF roman/params/submap_align_params.py:86-150].
        Aliases are rewritten in place like the reference (:93-96)."""
        fusion = {'geometric_mean': _abi.ROMAN_FUSE_GEOMETRIC_MEAN,
                  'arithmetic_mean': _abi.ROMAN_FUSE_ARITHMETIC_MEAN,
                  'product': _abi.ROMAN_FUSE_PRODUCT}.get(self.fusion_method)
        if self.method == 'spvg':
            self.method = 'roman'
        elif self.method == 'roman_no_semantics':
            self.method = 'pcavolgrav'

        if self.method in ['clipper', 'gravity', 'pcavolgrav', 'extentvolgrav', 'roman', 'sevg', 'spv', 'semanticgrav']:
            roman_params = ROMANParams()
            roman_params.point_dim = self.dim
            roman_params.sigma = self.sigma
            roman_params.epsilon = self.epsilon
            roman_params.mindist = self.mindist
            roman_params.fusion_method = fusion        # stored, never forwarded (reference behaviour)
            roman_params.gravity = self.method in ['gravity', 'pcavolgrav', 'extentvolgrav', 'roman', 'sevg', 'semanticgrav']
            roman_params.volume = self.method in ['pcavolgrav', 'extentvolgrav', 'roman', 'sevg', 'spv']
            roman_params.extent = self.method in ['extentvolgrav', 'sevg']
            roman_params.pca = self.method in ['pcavolgrav', 'roman', 'spv']
            roman_params.cos_min = self.cosine_min
            roman_params.cos_max = self.cosine_max
            roman_params.epsilon_shape = self.epsilon_shape
            roman_params.gravity_unc_ang_rad = self.gravity_unc_ang_rad
            if self.method in ['roman', 'sevg', 'semanticgrav']:
                roman_params.semantics_dim = self.semantics_dim
            registration = ROMANRegistration(roman_params)
        elif self.method == 'clipper+prune':
            registration = DistRegWithPruning(
                sigma=self.sigma, epsilon=self.epsilon, mindist=self.mindist,
                shape_epsilon=self.epsilon_shape, cos_min=self.cosine_min, dim=self.dim, use_gravity=True)
        elif self.method == 'ransac':
            # [REF roman/params/submap_align_params.py:145-147] builds RansacReg(dim=..., max_iteration=ransac_iter); the
            # reference's own constructor then raises TypeError ([REF roman/align/ransac_reg.py:14]) — this one runs
            registration = RansacReg(dim=self.dim, max_iteration=self.ransac_iter)
        else:
            assert False, "Invalid method"
        return registration
