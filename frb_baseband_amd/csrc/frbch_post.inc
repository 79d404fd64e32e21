// Empty: the code is in frbch_post.cpp.  The name stays for tests/emu/Makefile of earlier commits, which lists it as a prerequisite.
