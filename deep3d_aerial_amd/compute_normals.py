"""Drop-in for the reference's ComputeNormals (mvs/mvs_cas/models/compute_normals.py), DESIGN.md §1 row N5.

The reference defines the module and never calls it; its product is the {view}_normal.pfm the fusion step reads
(fuse/fusion_3d_normal.py:437-443, 491-498).  Here `compute_normal_by_depth` is one launch of d3d_normals_from_depth
(csrc/normals.hip) and `forward` keeps the reference's signature and layout.

* `compute_depth_by_normal` (:84-230) is not provided: it is unused in the reference and broken there -- the x1 / y1
  depths divide by `denominator_y0` (:148-149) and every `depth_*` map aliases `depth_init`, which is overwritten in
  place (:151-166), so the eight candidates are one array.
* `forward` resamples `img` with F.interpolate and never uses the result (:232): `img` is accepted and ignored.
* `torch.cross` without `dim` crosses along the first axis of size 3; for B * (H - 2 nei) * (W - 2 nei) == 3 the reference
  therefore crosses the wrong axis.  The kernel always crosses x, y, z.
"""
import torch

from . import ops


class ComputeNormals(torch.nn.Module):
    def __init__(self):
        super(ComputeNormals, self).__init__()

    def compute_normal_by_depth(self, depth_est, ref_intrinsics, nei):
        """depth_est [B,H,W], ref_intrinsics [B,3,3] -> camera-space normals [B,H,W,3] (border band of width nei = 0)."""
        return ops.normals_from_depth(depth_est.float().contiguous(), ref_intrinsics, nei=int(nei))

    def forward(self, init_depth, img, intri_matrices):
        """init_depth [B,H,W], img (unused), intri_matrices [B,V,3,3] -> [B,3,H,W] from view 0's intrinsics, nei = 1."""
        del img
        intrinsics = torch.unbind(intri_matrices, 1)[0]
        rough_normal = self.compute_normal_by_depth(init_depth, intrinsics, nei=1)
        return rough_normal.permute(0, 3, 1, 2)
