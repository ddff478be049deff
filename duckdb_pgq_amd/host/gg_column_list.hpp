// gg_column_list.hpp — the `columns` argument of gg_khop_extend_distinct: a comma-separated list of column numbers.
// Plain C++ without a duckdb header, so the parser can be compiled into a stand-alone program.
#pragma once

#include <string>
#include <vector>

namespace duckdb {

//! Parses "c0, c1, ..." — decimal numbers in 0..max_col, pairwise different, blanks allowed around them — into `out`.
//! false: `error` says what is wrong with the text (the caller names the argument).
inline bool GGParseColumnList(const std::string &text, int max_col, std::vector<int> &out, std::string &error) {
	out.clear();
	size_t i = 0;
	const size_t n = text.size();
	auto blanks = [&]() {
		while (i < n && (text[i] == ' ' || text[i] == '\t')) {
			i++;
		}
	};
	blanks();
	if (i == n) {
		error = "an empty list";
		return false;
	}
	while (true) {
		blanks();
		if (i == n || text[i] < '0' || text[i] > '9') {
			error = "a column number is expected at position " + std::to_string(i) + " of '" + text + "'";
			return false;
		}
		long value = 0;
		while (i < n && text[i] >= '0' && text[i] <= '9') {
			value = value * 10 + (text[i] - '0');
			if (value > max_col) { // (also keeps `value` from overflowing on a long run of digits)
				error = "a column outside 0.." + std::to_string(max_col) + " in '" + text + "'";
				return false;
			}
			i++;
		}
		for (int seen : out) {
			if (seen == (int)value) {
				error = "column " + std::to_string(value) + " is listed twice in '" + text + "'";
				return false;
			}
		}
		out.push_back((int)value);
		blanks();
		if (i == n) {
			return true;
		}
		if (text[i] != ',') {
			error = "a comma is expected at position " + std::to_string(i) + " of '" + text + "'";
			return false;
		}
		i++;
	}
}

} // namespace duckdb
