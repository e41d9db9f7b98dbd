# The host units of the engine (each includes kp_host.h): engine.cpp, and the ABI areas cut
# out of it into units of their own. The one list the builds take: this directory's Makefile
# and tools/sanitize/Makefile include it, and tools/variant_tu.sh reads it with
# `make -s print-units`.
HOST_UNITS = engine snapshot pack nodes answers watch assumed
