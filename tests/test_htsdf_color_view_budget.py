"""The register record of the new kernels of the coloured hashed views, compile only: num_vgpr and
private_seg_size are reported, and each new kernel must use no scratch if its dense counterpart uses none in the same build -- the dense
kernel is the yardstick.  k_htsdf_raycast_color and k_tsdf_raycast_color are templates: both instances of each are looked at."""
from device_asm import device_asm, kernel_resources

PAIRS = (("k_htsdf_raycast_color", "k_tsdf_raycast_color", 2), ("k_htm_colors", "k_tm_colors", 1))


def resources_of(seen, kernel, count):
    hits = [v for k, v in sorted(seen.items()) if k.startswith("_ZN6icpdev%d%sE" % (len(kernel), kernel)) or k.startswith("_ZN6icpdev%d%sILb" % (len(kernel), kernel))]
    assert len(hits) == count, (kernel, len(hits))
    return hits


def test_new_kernels_use_no_scratch_where_the_dense_ones_use_none():
    seen = kernel_resources(device_asm())
    for new, dense, count in PAIRS:
        for a, b in zip(resources_of(seen, new, count), resources_of(seen, dense, count)):
            print("%s: %d VGPRs, %d AGPRs, %d bytes of scratch (%s: %d VGPRs, %d bytes of scratch)" % (new, a["num_vgpr"], a["num_agpr"], a["private_seg_size"], dense,
                                                                                                        b["num_vgpr"], b["private_seg_size"]))
            if b["private_seg_size"] == 0:
                assert a["private_seg_size"] == 0, (new, a)
