"""CPU checks of the batched finder's ABI: lsm2d_find_correspondences_batch is declared by include/lsm2d.h, bound by the Python mirror with its eleven
arguments and exported by the gfx950 build; the two batched finder kernels are in the library's code object."""
import abi_checks


def test_find_batch_symbol_declared_bound_and_exported():
    abi_checks.assert_declared_bound_exported("lsm2d_find_correspondences_batch", 11)


def test_find_batch_kernels_are_in_the_code_object():
    abi_checks.assert_kernels_in_code_object((b"k_find_projective_batch", b"k_find_nn_batch"))


def test_finder_classes_have_compute_batch():
    from srrg2_laser_slam_2d_amd import api
    for cls in (api.CorrespondenceFinderProjective2f, api.CorrespondenceFinderKDTree2D, api.CorrespondenceFinderNN2D):
        assert callable(getattr(cls, "compute_batch"))
    assert abi_checks.assert_mirrors_have((), ("computeBatch(",)).count("computeBatch(") == 2
