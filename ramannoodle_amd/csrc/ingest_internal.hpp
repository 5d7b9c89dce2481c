// Internal entries of the trajectory readers (ingest.cpp, ingest_vasprun.cpp), not part of the C ABI
// of include/rn_ingest.h: rn_*_open is "map the file at this path" followed by "index this text".
// The second half is declared here so that a test program can hand the readers a buffer of exactly
// known size (tests/native/ingest_sweep.cpp: a heap copy under AddressSanitizer, where one byte past
// the end is a report; a mapped file has no such red zone behind it).
#pragma once
#include <stddef.h>

#include "../../include/rn_ingest.h"

extern "C" {

// Like rn_xdatcar_open / rn_vasprun_open on a file that holds text[0, size).  The handle keeps the
// pointer and does not own it: the text must stay alive and unchanged until rn_*_close.
int rn_xdatcar_open_text(const char *text, size_t size, rn_xdatcar **out);
int rn_vasprun_open_text(const char *text, size_t size, rn_vasprun **out);

}  // extern "C"
