"""CPU checks of the batched factor's ABI: lsm2d_linearize_batch is declared by include/lsm2d.h, bound by the Python mirror with its fourteen arguments and
exported by the gfx950 build; the three batch kernels are in the library's code object; the Python and the C++ mirror have their entries."""
import abi_checks


def test_linearize_batch_symbol_declared_bound_and_exported():
    abi_checks.assert_declared_bound_exported("lsm2d_linearize_batch", 14)


def test_linearize_batch_kernels_are_in_the_code_object():
    abi_checks.assert_kernels_in_code_object((b"k_linearize_partial_batch", b"k_linearize_final_batch", b"k_linearize_seq_batch"))


def test_mirrors_have_linearize_batch():
    abi_checks.assert_mirrors_have("linearize_batch", ("linearizeBatch(", "linearize(", "lsm2d_linearize_batch("))
