"""CPU checks of the batched-tracker ABI: the four entry points of N independent trackers per call are declared by include/lsm2d.h, bound
by the Python mirror and exported by the gfx950 build; the batched kernels are in the library's code object."""
import abi_checks

NEW = {"lsm2d_cloudset_create_reserved_many": None, "lsm2d_cloudset_clear_clouds": None, "lsm2d_clip_scene_batch": 9, "lsm2d_merge_scene_batch": 12}


def test_batch_symbols_declared_bound_and_exported():
    for name, n_args in NEW.items():
        abi_checks.assert_declared_bound_exported(name, n_args)


def test_batch_kernels_are_in_the_code_object():
    abi_checks.assert_kernels_in_code_object((b"k_clip_batch", b"k_merge_batch"))
