"""CPU check: a decoder pool whose shared-memory segment a consumer page-locked (eval_driver._pin_pool_memory) undoes
that registration on close() while the segment is still mapped."""
from multiprocessing import shared_memory

import pytest

from scene_3dreconstruction_mvsnet_amd.decoder_pool import DecoderPool, ViewDecoderPool


@pytest.mark.parametrize("cls", [DecoderPool, ViewDecoderPool])
def test_close_unpins_before_unmapping(cls):
    pool = cls(None, procs=1)
    shm = pool._shm = shared_memory.SharedMemory(create=True, size=4096)
    seen = []
    pool._unpin = lambda: seen.append(shm.buf is not None)   # still mapped when called
    pool.close()
    assert seen == [True] and pool._shm is None and "_unpin" not in pool.__dict__
