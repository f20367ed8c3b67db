// The CLI's side outputs: coverage, pileup, structural-variant signatures and error profile. Each keeps one library object per device
// context, is fed with every run that context aligns, and after the last batch sums the objects into the first and writes its text
// file(s) from there. (PAF and SAM/BAM are not of this kind: they take the copied records in input order, on the writer thread.)
#pragma once
#include <memory>
#include <vector>

#include "../../include/floxer_amd.h"
#include "cli_input.hpp"
#include "cli_options.hpp"

struct SideOutput {
    virtual ~SideOutput() = default;                                               // frees the objects: before their contexts are destroyed
    // the run of a batch that context number `slot` aligned; the library's code (flx_last_error() holds the text, on this thread)
    virtual int add(size_t slot, const flx_run* run, ReadBatch const& batch) = 0;
    virtual bool write() = 0;                                                      // false behind the error line
};

// The side outputs the options ask for, in the one order they are created, fed and written in: coverage, pileup, sv, error profile.
// False behind the error line when an object cannot be set up.
bool make_side_outputs(Options const& o, std::vector<flx_ctx*> const& ctxs, Reference const& ref, std::vector<std::unique_ptr<SideOutput>>& list);
