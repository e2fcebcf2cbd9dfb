"""The register record of the two accumulate kernels of a laser scan's direct SDF alignment, compile only: num_vgpr
and private_seg_size are reported next to those of the depth form's kernels, and neither new kernel may have a private segment (the 28
fp64 sums of a lane, the eight corners and, on the hashed volume, up to eight block indices all have to stay in registers)."""
from device_asm import device_asm, kernel_resources

NEW = ("k_sdf_accumulate_cloud", "k_hsdf_accumulate_cloud")
BESIDE = ("k_sdf_accumulate", "k_hsdf_accumulate", "k_vgicp_accumulate")


def resources_of(seen, kernel):
    hits = [v for k, v in seen.items() if k.startswith("_ZN6icpdev%d%sE" % (len(kernel), kernel))]
    assert len(hits) == 1, (kernel, len(hits))
    return hits[0]


def test_the_cloud_accumulates_use_no_scratch():
    seen = kernel_resources(device_asm())
    for k in BESIDE + NEW:
        a = resources_of(seen, k)
        print("%s: %d VGPRs, %d AGPRs, %d bytes of scratch" % (k, a["num_vgpr"], a["num_agpr"], a["private_seg_size"]))
    for new in NEW:
        a = resources_of(seen, new)
        assert a["private_seg_size"] == 0, (new, a)
        assert a["num_vgpr"] + a["num_agpr"] <= 256, (new, a)      # (at least two waves per SIMD of 512 registers per lane)
