// The CLI's log lines: "[floxer] [level] text" on stderr (debug lines only with -c/--console-debug-logs) and "[level] text" in the log file.
#pragma once
#include <cstdarg>
#include <cstdio>
#include <cstring>

inline bool g_debug = false;
inline FILE* g_logfile = nullptr;

inline void log_line(const char* level, const char* fmt, ...) {
    char buf[4096];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    bool const is_debug = strcmp(level, "debug") == 0;
    if (!is_debug || g_debug) fprintf(stderr, "[floxer] [%s] %s\n", level, buf);
    if (g_logfile) { fprintf(g_logfile, "[%s] %s\n", level, buf); fflush(g_logfile); }
}
