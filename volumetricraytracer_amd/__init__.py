"""MI355X-native volumetric SDF ray-marcher behind the VRenderer surface of
Elyptos/VolumetricRaytracer.  The product is the C-ABI library built from csrc/ (see
include/vrt.h); this package is its host-side mirror of the reference's scene types."""
from . import _abi
from .renderer import (CONTACT_DTYPE, HIT_DTYPE, POINT_DTYPE, POINT_RESULT_DTYPE, RAY_DTYPE, SWEEP_DTYPE, SWEEP_HIT_DTYPE, VHipRenderer, algorithmic_bytes, box_brush,
                       capsule_brush, contacts_to_dict, hits_to_dict, make_points, make_rays, make_sweeps, point_results_to_dict, smooth_record, sphere_brush,
                       stamp_from_placement, stamp_record, sweep_hits_to_dict, warp_from_motion, warp_record)
from .scene import (ADD, FORWARD, IDENTITY, RIGHT, SUBTRACT, UP, VBox, VCamera, VCylinder, VDensityGenerator,
                    VLight, VMaterial, VPointLight, VScene, VSphere, VSpotLight, VVoxelObject, VVoxelVolume,
                    csg_volume, default_params, demo_light, march_budget, look_minus_x_camera, procedural_skybox,
                    quat_from_axis_angle, quat_from_euler_deg, quat_inverse, quat_mul, quat_rotate, sphere_volume,
                    torus_volume)

__all__ = [n for n in dir() if not n.startswith("_")] + ["_abi"]
