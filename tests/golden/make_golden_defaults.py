"""The reference's config DEFAULTS (MQ/libs/core/config.py), recorded from the IMPORTED REFERENCE so that
tests/test_cabi_cpu.py compares the config surface with it without the reference tree.
Run:  python tests/golden/make_golden_defaults.py  ->  tests/golden/config_defaults.pt"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import  # noqa: E402


def main():
    libs = ref_import.setup()
    torch.save(libs.core.config.DEFAULTS, os.path.join(HERE, "config_defaults.pt"))


if __name__ == "__main__":
    main()
