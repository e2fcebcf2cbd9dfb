"""The register record of the five kernels of the cloud integrate, compile only: num_vgpr and private_seg_size
are reported, and each new kernel must use no scratch if k_htsdf_touch -- the depth frame's walk, the shape they follow -- uses none in
the same build."""
from device_asm import device_asm, kernel_resources

NEW = ("k_htsdf_touch_cloud", "k_htsdf_accumulate_cloud", "k_tsdf_accumulate_cloud", "k_htsdf_fold_cloud", "k_tsdf_fold_cloud")
YARDSTICK = "k_htsdf_touch"


def resources_of(seen, kernel):
    hits = [v for k, v in seen.items() if k.startswith("_ZN6icpdev%d%sE" % (len(kernel), kernel))]
    assert len(hits) == 1, (kernel, len(hits))
    return hits[0]


def test_new_kernels_use_no_scratch_where_the_depth_touch_uses_none():
    seen = kernel_resources(device_asm())
    b = resources_of(seen, YARDSTICK)
    for new in NEW:
        a = resources_of(seen, new)
        print("%s: %d VGPRs, %d AGPRs, %d bytes of scratch (%s: %d VGPRs, %d bytes of scratch)" % (new, a["num_vgpr"], a["num_agpr"], a["private_seg_size"], YARDSTICK,
                                                                                                    b["num_vgpr"], b["private_seg_size"]))
        if b["private_seg_size"] == 0:
            assert a["private_seg_size"] == 0, (new, a)
