"""The register record of the four kernels of the coloured cloud fuse, compile only: num_vgpr and private_seg_size of
the colour accumulates are reported beside the geometry accumulate each follows, those of the colour folds beside the geometry folds, and
none may use a private segment."""
from device_asm import device_asm, kernel_resources

NEW = ("k_htsdf_accumulate_cloud_color", "k_tsdf_accumulate_cloud_color", "k_htsdf_fold_cloud_color", "k_tsdf_fold_cloud_color")
BESIDE = ("k_htsdf_accumulate_cloud", "k_tsdf_accumulate_cloud", "k_htsdf_fold_cloud", "k_tsdf_fold_cloud")


def resources_of(seen, kernel):
    hits = [v for k, v in seen.items() if k.startswith("_ZN6icpdev%d%sE" % (len(kernel), kernel))]
    assert len(hits) == 1, (kernel, len(hits))
    return hits[0]


def test_colour_kernels_use_no_scratch():
    seen = kernel_resources(device_asm())
    for new, old in zip(NEW, BESIDE):
        a, b = resources_of(seen, new), resources_of(seen, old)
        print("%s: %d VGPRs, %d AGPRs, %d bytes of scratch (%s: %d VGPRs, %d bytes of scratch)" % (new, a["num_vgpr"], a["num_agpr"], a["private_seg_size"], old, b["num_vgpr"],
                                                                                                    b["private_seg_size"]))
        assert a["private_seg_size"] == 0, (new, a)
