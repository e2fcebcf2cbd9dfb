"""The register record of the two coloured accumulate kernels of a laser scan's direct SDF alignment, compile only:
num_vgpr and private_seg_size are reported next to those of the geometric cloud kernels and of the depth form's coloured kernels, and
neither new kernel may have a private segment (the 29 fp64 sums of a lane, the two rows' Jacobians, sixteen corners and, on the hashed
volume, up to eight block indices all have to stay in registers) or more than 256 registers per lane (two waves per SIMD)."""
from device_asm import device_asm, kernel_resources

NEW = ("k_sdf_accumulate_cloud_color", "k_hsdf_accumulate_cloud_color")
BESIDE = ("k_sdf_accumulate_cloud", "k_hsdf_accumulate_cloud", "k_sdf_accumulate_color", "k_hsdf_accumulate_color")


def resources_of(seen, kernel):
    hits = [v for k, v in seen.items() if k.startswith("_ZN6icpdev%d%sE" % (len(kernel), kernel))]
    assert len(hits) == 1, (kernel, len(hits))
    return hits[0]


def test_the_coloured_cloud_accumulates_use_no_scratch():
    seen = kernel_resources(device_asm())
    for k in BESIDE + NEW:
        a = resources_of(seen, k)
        print("%s: %d VGPRs, %d AGPRs, %d bytes of scratch" % (k, a["num_vgpr"], a["num_agpr"], a["private_seg_size"]))
    for new in NEW:
        a = resources_of(seen, new)
        assert a["private_seg_size"] == 0, (new, a)
        assert a["num_vgpr"] + a["num_agpr"] <= 256, (new, a)      # (at least two waves per SIMD of 512 registers per lane)
