"""The register record of the three new kernels of the coloured hashed volume, compile only: num_vgpr and
private_seg_size are reported, and each new kernel must use no scratch if its dense counterpart uses none in the same build -- the dense
kernel is the yardstick."""
from device_asm import device_asm, kernel_resources

PAIRS = (("k_htsdf_integrate_color", "k_tsdf_integrate_color"), ("k_htsdf_sample_color", "k_tsdf_sample_color"), ("k_hsdf_accumulate_color", "k_sdf_accumulate_color"))


def resources_of(seen, kernel):
    hits = [v for k, v in seen.items() if k.startswith("_ZN6icpdev%d%sE" % (len(kernel), kernel))]
    assert len(hits) == 1, (kernel, len(hits))
    return hits[0]


def test_new_kernels_use_no_scratch_where_the_dense_ones_use_none():
    seen = kernel_resources(device_asm())
    for new, dense in PAIRS:
        a, b = resources_of(seen, new), resources_of(seen, dense)
        print("%s: %d VGPRs, %d AGPRs, %d bytes of scratch (%s: %d VGPRs, %d bytes of scratch)" % (new, a["num_vgpr"], a["num_agpr"], a["private_seg_size"], dense,
                                                                                                    b["num_vgpr"], b["private_seg_size"]))
        if b["private_seg_size"] == 0:
            assert a["private_seg_size"] == 0, (new, a)
