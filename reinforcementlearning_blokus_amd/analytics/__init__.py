"""Analytics on top of the GPU engine (reference: analytics/)."""
