#!/usr/bin/env python3
"""Regenerate every committed tw_h?*_asm.inc / *_clobbers.inc under timewarp_amd/csrc from the generators: the rows of
tools/h3_asm_manifest.py, which tests/test_host_logic.py::test_generated_asm_includes_are_current checks the committed text against."""
import h3_asm_manifest as manifest

for row in manifest.ROWS:
    manifest.run(row)
print(f"{len(manifest.ROWS)} statements")
