"""BrotliMi355xCompressBatchWithDictionariesDevice with an image per frequently named dictionary: the mixed group of
test_batch_dictionaries_images with dictionaries and items in device memory.  A group builds its images from the copy of each
dictionary that the staging launch has put in front of the first item that names it, so the device form makes no copy of its own.
The bytes, last_batch_info() and last_batch_image_info() are those of the host call on the same bytes.  One more item lies inside
its own dictionary's allocation: inputs and dictionaries may overlap.  Built like test_batch_dictionaries_device (the emulation
library takes host addresses for device addresses)."""
import pytest

import test_cabi
from test_batch_dictionaries_device import _Layout, _call, _host, _mem, _oracle, _place, _roomy
from test_batch_dictionaries_images import _mixed_group


def _mixed_on_device(which, quality, lgwin, quick):
    lib, Mem = test_cabi._load(which), _mem(which)
    items, dictionaries, named = (list(x) for x in _mixed_group())
    inside = dictionaries[0][300:1100]  # lies inside dictionary A's allocation, and names A
    items.append(inside)
    named.append(0)
    dict_blocks = _place(dictionaries, 3)
    item_blocks = _place(items[:-1], dict_blocks[-1][0] + len(dict_blocks[-1][1]) + 1) + [(dict_blocks[0][0] + 300, inside)]
    lay = _Layout(Mem, dict_blocks + item_blocks, _roomy(lib, items))
    sizes, info, error = _call(lib, lay, dict_blocks, item_blocks, named, quality, lgwin, quick)
    images = lib.last_batch_image_info()
    assert error is None, error
    got = lay.streams(sizes)
    for i, (g, x, k) in enumerate(zip(got, items, named)):
        assert g == _oracle(x, quality, lgwin, dictionaries[k]), (quality, lgwin, i, len(x), k)
    want, host_info = _host(lib, dictionaries, items, named, quality, lgwin, quick)
    assert got == want and info == host_info, (info, host_info)
    assert info[1] == len(items) and info[4] == 1, info
    assert images == lib.last_batch_image_info() == [4, 114, 3, 0], (images, lib.last_batch_image_info())
    assert lay.src.read() == lay.before and lay.untouched_outside(sizes)


_CASES = [(5, 22, False), (2, 22, True)]
_CASE_IDS = ["q5", "q2-quick"]


@pytest.mark.parametrize("quality,lgwin,quick", _CASES, ids=_CASE_IDS)
def test_mixed_group_on_device_emu(quality, lgwin, quick):
    _mixed_on_device("emu", quality, lgwin, quick)


@pytest.mark.gpu
@pytest.mark.parametrize("quality,lgwin,quick", _CASES, ids=_CASE_IDS)
def test_mixed_group_on_device_gpu(quality, lgwin, quick):
    _mixed_on_device("gpu", quality, lgwin, quick)
