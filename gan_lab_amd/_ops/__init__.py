"""The op families behind ``gan_lab_amd.ops``: one module per family of ``csrc/*.hip`` launchers, ``core`` for what they share.
Callers import ``gan_lab_amd.ops``, which re-exports every name; no module here imports it."""
