"""How a weight-prefetch target is dealt over the waves that touch it (msd_op_touch_deal: host only, no GPU).  The same
function deals the in-block prefetch waves and the touch blocks of a carrier launch (csrc/gemm_h16.h touch_first_row),
so what holds here holds for both device forms: every 128-byte line of the target is touched exactly once and no touch
lies beyond the target."""
import ctypes
import os
import re

import numpy as np
import pytest

from msd_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = 128
WAVES = (1, 5, 64 * 4)
# (rows, row_bytes, row_pitch): one line; 127 and 129 lines, one per row; a 2-D range whose rows are 200 bytes (a line and
# a part of one) 256 apart; and the same with rows of three lines and a tail inside a wider matrix
TARGETS = {'1 line': (1, 128, 128), '127 lines': (127, 128, 128), '129 lines': (129, 128, 128),
           '2-D, 200-byte rows': (10, 200, 256), '2-D, 330-byte rows in a 1 KiB pitch': (37, 330, 1024)}
NEW_SYMBOLS = ('msd_op_touch_deal', 'msd_op_gemm_site_carrier', 'msd_op_attention_launch_carrier', 'msd_set_touch_carrier')


@pytest.fixture(scope='module')
def lib():
  import __graft_entry__
  __graft_entry__.build()
  return native.load()


def _target_bytes(rows, row_bytes, pitch):
  return (rows - 1) * pitch + row_bytes


@pytest.mark.parametrize('waves', WAVES)
@pytest.mark.parametrize('name', sorted(TARGETS))
def test_every_line_once_and_nothing_beyond_the_target(lib, name, waves):
  rows, row_bytes, pitch = TARGETS[name]
  total = _target_bytes(rows, row_bytes, pitch)
  deal = native.op_touch_deal(total, row_bytes, pitch, waves)
  assert deal.shape[0] == waves and deal.shape[2] == 3
  lines_per_row = -(-row_bytes // LINE)
  seen = np.zeros((rows, lines_per_row), np.int64)
  for w in range(waves):
    for r0, n, lpr in deal[w]:
      if n == 0:
        continue
      assert lpr == lines_per_row and 0 <= r0 and r0 + n <= rows, (w, r0, n, lpr)
      # a touch is 4 bytes at the start of a line: the last byte read lies inside the row, so inside the target
      last = (r0 + n - 1) * pitch + (lpr - 1) * LINE + 3
      assert last < total and (lpr - 1) * LINE + 3 < row_bytes, (w, r0, n, last, total)
      seen[r0:r0 + n] += 1
  assert (seen == 1).all(), 'lines touched %s times' % sorted(set(seen.ravel().tolist()))


def test_a_wave_deals_whole_touches_block_cyclically(lib):
  """Touch u of wave w starts at row (w + waves * u) * rows-per-touch: 64 lanes = 64 >> lg rows of 2^lg line slots."""
  deal = native.op_touch_deal(_target_bytes(1900, 256, 256), 256, 256, 5)   # two lines per row: 32 rows per touch
  per_wave = deal.shape[1]
  for w in range(5):
    for u in range(per_wave):
      assert deal[w, u, 0] == (w + 5 * u) * 32


def test_a_target_the_waves_cannot_cover_is_refused(lib):
  deal = native.op_touch_deal(_target_bytes(64, 128, 128), 128, 128, 1)
  per_wave = deal.shape[1]
  rows = per_wave * 64 + 1          # one row more than one wave's touches hold
  buf = (ctypes.c_int32 * (per_wave * 3))()
  assert lib.msd_op_touch_deal(_target_bytes(rows, 128, 128), 128, 128, 1, buf, len(buf)) == -6   # MSD_ERR_UNSUPPORTED
  assert lib.msd_op_touch_deal(_target_bytes(rows - 1, 128, 128), 128, 128, 1, buf, len(buf)) == per_wave
  # bad arguments: no waves, a pitch below the row, a target that is no whole number of rows, a buffer too small
  assert lib.msd_op_touch_deal(128, 128, 128, 0, buf, len(buf)) == -1
  assert lib.msd_op_touch_deal(128, 128, 64, 1, buf, len(buf)) == -1
  assert lib.msd_op_touch_deal(300, 128, 128, 1, buf, len(buf)) == -1
  assert lib.msd_op_touch_deal(128, 128, 128, 2, buf, len(buf)) == -1


def test_knob_and_entries_in_header_binding_and_both_libraries(lib):
  text = open(os.path.join(ROOT, 'include', 'msd_amd.h')).read()
  code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
  declared = set(re.findall(r'\b(msd_[a-z0-9_]+)\s*\(', code))
  for planes in ('f16', 'bf16'):
    other = native.load(planes)
    for name in NEW_SYMBOLS:
      assert name in declared and name in native.EXPORTED_SYMBOLS and hasattr(other, name), (planes, name)
  # the knob is the LAST field of msd_config, behind ABI 6's: a caller that does not know it passes ABI 6's size
  assert native.MsdConfig._fields_[-1][0] == 'touch_carrier'
  assert native.ABI_STRUCT_SIZES[7] == native.MsdConfig.touch_carrier.offset
  assert native.config_struct_size(lib) == ctypes.sizeof(native.MsdConfig)
  assert lib.msd_set_touch_carrier(None, 1) == 1 and lib.msd_create(None, None) == 1   # MSD_ERR_INVALID_ARGUMENT, no device


def test_inference_keyword_reaches_the_config():
  import msd_amd
  from msd_amd import inference
  spec = msd_amd.config.preset('tiny_context', num_steps=8)
  codec = msd_amd.audio_codecs.get_codec(spec.audio_codec)
  for value, want in ((None, 0), (1, 1), (2, 2)):
    cfg = inference._to_native_config(spec, codec, 1, 'f16x3', touch_carrier=value)
    assert cfg.touch_carrier == want
  with pytest.raises(ValueError):
    inference._to_native_config(spec, codec, 1, 'f16x3', touch_carrier=0)
