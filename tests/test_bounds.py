"""Where the generic kernels write: the cases of tests/bounds_cases.py that a build without the hand-written kernels can run,
through the TEST-ONLY emulator build on guarded host buffers (tests/hipmem.py::HostGuardedBuffer) -- outputs of exactly the
documented size between two guard bands, poisoned before the call; inputs checksummed; a second call into the dirty output.
The same table runs on the device in tests/test_gpu_bounds.py, where the hand-written kernels meet it."""
import pytest

from tests import bounds_cases as bc
from tests.hipmem import HostGuardedBuffer, guarded_for


def test_the_checker_sees_one_byte_on_either_side_and_in_an_input():
    bc.checker_self_test(HostGuardedBuffer)


@pytest.mark.parametrize("name", bc.ids(emu_only=True))
def test_generic_kernels_write_inside_their_buffers(emu_lib, name):
    assert guarded_for(emu_lib) is HostGuardedBuffer
    bc.run(emu_lib, name)
