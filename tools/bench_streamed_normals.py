"""bench.py with RDYHIP_CONFIG_STREAMED_NORMALS set on every operator it creates: the third leg of the normal table's A/B (this
build's streamed family, which must show the parent's time).  usage: python tools/bench_streamed_normals.py [bench arguments]"""
import dataclasses
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rdycore_amd import operator as O  # noqa: E402

_abi_arguments = O._abi_arguments      # what every create and probe turns its RDyFlowConfig into the C structs with


def _streamed(config, mesh, condition_types):
    return _abi_arguments(dataclasses.replace(config, streamed_normals=True), mesh, condition_types)


O._abi_arguments = _streamed
sys.argv[0] = os.path.join(ROOT, "bench.py")
runpy.run_path(sys.argv[0], run_name="__main__")
